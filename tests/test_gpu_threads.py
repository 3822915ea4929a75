"""Several host threads in the C ABI at once (the reference's concurrency contract, J/README.md:11): 4 threads, each on an
input of its own, compress, decompress and batch-compress with Bzip2 and compress and decompress with BWTC through the
host-buffer entry points and free the results, three times over.  Every result must equal the one the same call gave on a
single thread.  Results of 1 MiB and more come from the pinned result pool, so this runs cjs_free and the pool's take / give
from several threads at once.  The same threaded run is repeated in fresh processes under pool settings that make every give
evict (the settings are read once per process).  A pass does not prove that no race is left; it is the contract under load."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import recipes
import support

pytestmark = pytest.mark.gpu

THREADS = 4
REPEATS = 3
INPUT_BYTES = 6_000_000                 # level-9 stream of textgen text: well over 1 MiB (pinned result path)
BATCH_SIZES = (1, 300, 70_000, 250_000)
# fresh-process variants: (a) no idle device buffers are kept and at most 1 MiB of idle pinned results, so every give evicts;
# (b) results are plain malloc and no context is cached
VARIANTS = {
    "evict": {"CJS_DEVICE_POOL_MB": "0", "CJS_PINNED_RESULT_MB": "1"},
    "no_cache": {"CJS_PINNED_RESULT_MB": "0", "CJS_NO_CTX_CACHE": "1"},
}


def _lib():
    h = support.HipLib()
    L = h.L
    S = ctypes.c_size_t
    L.cjs_bzip2_compress_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(S), S, ctypes.c_int,
                                           ctypes.POINTER(support.u8p), ctypes.POINTER(S), ctypes.POINTER(S), ctypes.c_void_p]
    L.cjs_bzip2_compress_batch.restype = ctypes.c_int
    return h


def _batch(h, inputs):
    """cjs_bzip2_compress_batch of `inputs` -> (rc, [stream bytes])"""
    count = len(inputs)
    ptrs = (ctypes.c_void_p * count)(*[x.ctypes.data for x in inputs])
    ns = (ctypes.c_size_t * count)(*[x.size for x in inputs])
    off = (ctypes.c_size_t * count)()
    ln = (ctypes.c_size_t * count)()
    out = support.u8p()
    rc = h.L.cjs_bzip2_compress_batch(ptrs, ns, count, 9, ctypes.byref(out), off, ln, None)
    if rc:
        return rc, None
    end = max(off[k] + ln[k] for k in range(count))
    buf = np.ctypeslib.as_array(out, shape=(max(end, 1),))
    streams = [buf[off[k]: off[k] + ln[k]].tobytes() for k in range(count)]
    h.L.cjs_free(out)
    return 0, streams


def _work(h, data, small):
    """one round of the calls a thread makes: (compressed, decompressed, batch streams, BWTC compressed, BWTC decompressed)"""
    rc, comp = h.bzip2_compress(data, 9)
    assert rc == 0, h.L.cjs_strerror(rc)
    rc, back = h.bzip2_decompress(comp)
    assert rc == 0, h.L.cjs_strerror(rc)
    rc, streams = _batch(h, small)
    assert rc == 0, h.L.cjs_strerror(rc)
    rc, wcomp = h.bwtc_compress(data, 9)
    assert rc == 0, h.L.cjs_strerror(rc)
    rc, wback = h.bwtc_decompress(wcomp)
    assert rc == 0, h.L.cjs_strerror(rc)
    return comp.tobytes(), back.tobytes(), streams, wcomp.tobytes(), wback.tobytes()


def _inputs():
    inputs = [recipes.textgen(INPUT_BYTES, 500 + t) for t in range(THREADS)]
    smalls = [[recipes.textgen(n, 900 + 10 * t + i) for i, n in enumerate(BATCH_SIZES)] for t in range(THREADS)]
    return inputs, smalls


def _digest(result):
    """sha256 of every bytes object of one _work result, in order"""
    comp, back, streams, wcomp, wback = result
    return [hashlib.sha256(x).hexdigest() for x in [comp, back] + streams + [wcomp, wback]]


def _threaded(h, inputs, smalls):
    """THREADS threads, REPEATS rounds of _work each -> (per thread: the rounds' results, errors)"""
    got = [[] for _ in range(THREADS)]
    errors = []

    def run(t):
        try:
            for _ in range(REPEATS):
                got[t].append(_work(h, inputs[t], smalls[t]))
        except BaseException as e:      # reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(THREADS)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    return got, errors


def _single(h, inputs, smalls):
    want = [_work(h, inputs[t], smalls[t]) for t in range(THREADS)]
    for t in range(THREADS):
        assert len(want[t][0]) >= 1 << 20
        assert want[t][1] == inputs[t].tobytes()
        assert want[t][4] == inputs[t].tobytes()
    return want


def test_host_abi_from_several_threads():
    h = _lib()
    inputs, smalls = _inputs()
    want = _single(h, inputs, smalls)                                       # single thread first
    got, errors = _threaded(h, inputs, smalls)
    assert not errors, errors
    for t in range(THREADS):
        assert len(got[t]) == REPEATS
        for r in range(REPEATS):
            comp, back, streams, wcomp, wback = got[t][r]
            assert comp == want[t][0], "thread %d round %d: compressed stream differs" % (t, r)
            assert back == want[t][1], "thread %d round %d: decompressed bytes differ" % (t, r)
            assert streams == want[t][2], "thread %d round %d: batch streams differ" % (t, r)
            assert wcomp == want[t][3], "thread %d round %d: BWTC stream differs" % (t, r)
            assert wback == want[t][4], "thread %d round %d: BWTC decompressed bytes differ" % (t, r)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_host_abi_from_several_threads_pool_settings(variant):
    h = _lib()
    inputs, smalls = _inputs()
    want = [_digest(w) for w in _single(h, inputs, smalls)]                 # in this process, default settings
    env = dict(os.environ, **VARIANTS[variant])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-4000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert not res["errors"], res["errors"]
    for t in range(THREADS):
        assert len(res["got"][t]) == REPEATS
        for r in range(REPEATS):
            assert res["got"][t][r] == want[t], "%s: thread %d round %d differs from the single-thread results" % (variant, t, r)


if __name__ == "__main__":      # the threaded run of a fresh process (test_host_abi_from_several_threads_pool_settings)
    try:        # one HIP runtime per process: torch's copy first, as in tests/conftest.py
        import torch  # noqa: F401
    except Exception:
        pass
    got, errors = _threaded(_lib(), *_inputs())
    print(json.dumps({"got": [[_digest(x) for x in g] for g in got], "errors": errors}))
