"""The five Bzip2 decode entry points on the same inputs: cjs_bzip2_decompress, cjs_bzip2_decompress_device,
cjs_bzip2_decompress_batch (all inputs as one batch), cjs_bzip2_decompress_batch_device and the streaming decoder fed 64 KiB at a
time give the same status, the same detail text and the same bytes, and each equals the oracle's decoder.  The inputs are the
smallest at which the glue the five share (header check, chain walk, verdict rule, output offsets) can go wrong.

A failed input has no bytes in the four one-shot forms.  The streaming decoder has by then delivered the blocks in front of the
failure, as its contract says: its bytes are then required to be a prefix of the intact stream's plain bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import recipes
import support
import test_gpu_dec_device as dd
import test_gpu_dec_stream as ds

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 65536


def _flip(stream, bit):
    out = stream.copy()
    out[bit >> 3] ^= 0x80 >> (bit & 7)
    return out


def build_inputs(oracle):
    """-> [(name, stream, plain bytes of the intact stream it was made from)]"""
    text = recipes.textgen(250000, 41)
    rc, s = oracle.bzip2_compress(text, 1)
    assert rc == 0
    rc, tab = oracle.bzip2_table(s, 0)
    assert rc == 0 and len(tab) == 3                                  # three blocks
    t1, t2 = recipes.textgen(120000, 42), recipes.textgen(230000, 43)
    m1, m2 = oracle.bzip2_compress(t1, 1)[1], oracle.bzip2_compress(t2, 2)[1]
    ms = np.concatenate([m1, m2])
    both = np.concatenate([t1, t2])

    def second_header(b):
        out = ms.copy()
        out[m1.size: m1.size + 4] = np.frombuffer(b, np.uint8)
        return out
    return [
        ("three blocks", s, text),
        ("block 2 crc", _flip(s, tab[1][0] + 48 + 5), text),          # the stored CRC follows the 48-bit block magic
        ("stream crc", _flip(s, s.size * 8 - 12), text),
        ("cut in block 3", s[: (tab[2][0] >> 3) + 5000], text),
        ("two members", ms, both),
        ("member 2 BZh0", second_header(b"BZh0"), both),
        ("member 2 BZx2", second_header(b"BZx2"), both),
        ("3 bytes", s[:3], text),
        ("BZx9", np.concatenate([np.frombuffer(b"BZx9", np.uint8), s[4:]]), text),
        ("BZh0", np.concatenate([np.frombuffer(b"BZh0", np.uint8), s[4:]]), text),
        ("empty stream", np.frombuffer(bytes.fromhex("425a683917724538509000000000"), np.uint8), np.empty(0, np.uint8)),
    ]


@pytest.fixture(scope="module")
def pkg():
    return dd._pkg()


@pytest.fixture(scope="module")
def inputs(oracle):
    return build_inputs(oracle)


def check_all(L, pkg, oracle, inputs, multi, streaming=True):
    """every entry point against cjs_bzip2_decompress and the oracle; returns {name: (status, bytes, detail)}"""
    streams = [x for _, x, _ in inputs]
    want = [dd.host(L, x, multi) for x in streams]                    # (status, bytes, detail)
    for (name, x, plain), w in zip(inputs, want):
        orc, obytes = oracle.bzip2_decompress(x, multi)
        assert w[0] == orc, (name, multi, w[0], orc)
        if orc == 0:
            assert w[1] == obytes.tobytes(), (name, multi)
        else:
            assert w[1] == b"", (name, multi)
        # (room for whatever a damaged stream decodes to before its verdict: a size above the capacity is -33 first, by contract)
        got = dd.device(L, x, multi, cap=max(plain.size, 8 * x.size) + 65536)
        assert got[:3] == w, (name, multi, "device", got[0], got[2], w[0], w[2])
        if streaming:
            rc, detail, b = ds.decode(pkg, x, multi, chunk=CHUNK, writes=[CHUNK] * (x.size // CHUNK) + [x.size % CHUNK])
            assert (rc, detail) == (w[0], w[2]), (name, multi, "stream", rc, detail, w[0], w[2])
            if rc == 0:
                assert b.tobytes() == w[1], (name, multi, "stream")
            else:
                assert b.size <= plain.size and np.array_equal(b, plain[: b.size]), (name, multi, "stream bytes before the failure")
    first_bad = next((w[2] for w in want if w[0]), "")
    rc, res, detail = dd.host_batch(L, streams, multi)
    assert rc == 0 and detail == first_bad, ("batch", multi, rc, detail, first_bad)
    rcd, resd, detaild, need, out = dd.device_batch(L, streams, multi, cap=sum(max(p.size, 8 * x.size) for _, x, p in inputs) + 65536)
    assert rcd == 0 and detaild == first_bad, ("batch device", multi, rcd, detaild, first_bad)
    assert bool((out[need:] == 0xA5).all())
    for k, ((name, _, _), w) in enumerate(zip(inputs, want)):
        for form, r in (("batch", res[k]), ("batch device", resd[k])):
            assert (r[0], r[3]) == (w[0], w[1]) and r[2] == len(w[1]), (name, multi, form, r[:3], w[0], len(w[1]))
    return dict(zip([n for n, _, _ in inputs], want))


@pytest.mark.parametrize("multi", [0, 1])
def test_five_entry_points_agree(oracle, pkg, inputs, multi):
    want = check_all(dd._lib(), pkg, oracle, inputs, multi)
    codes = {n: w[0] for n, w in want.items()}
    details = {n: w[2] for n, w in want.items()}
    assert codes["three blocks"] == 0 and codes["two members"] == 0 and codes["empty stream"] == 0
    assert codes["block 2 crc"] == -5 and codes["stream crc"] == -5 and codes["cut in block 3"] != 0
    assert codes["3 bytes"] == -2 and codes["BZx9"] == -2 and codes["BZh0"] == -2
    # the restart header is read only by a multistream decode
    assert codes["member 2 BZh0"] == codes["member 2 BZx2"] == (-2 if multi else 0)
    assert details["block 2 crc"].startswith("Bad block CRC (got ") and details["stream crc"].startswith("Bad stream CRC (got ")
    assert details["3 bytes"] == details["BZx9"] == "bad magic" and details["BZh0"] == "level out of range"
    if multi:
        assert details["member 2 BZh0"] == "level out of range" and details["member 2 BZx2"] == "bad magic"


_SHRUNK = r"""
import sys, numpy as np
sys.path.insert(0, "tests"); sys.path.insert(0, ".")
import torch; torch.zeros(1, device="cuda")      # (CUDA up in torch before the library's first call)
import support, test_gpu_dec_device as dd, test_gpu_dec_entry_parity as t
L = dd._lib(); o = support.Oracle()
ins = t.build_inputs(o)
rng = np.random.default_rng(5)
plain = rng.integers(0, 256, 300000, dtype=np.uint8)
_, big = o.bzip2_compress(plain, 1)                # larger than a group: the single path inside the batch
assert big.size > 200000 and max(x.size for _, x, _ in ins) <= 200000
ins[3:3] = [("oversized", big, plain), ("oversized, damaged", t._flip(big, 8 * 150000 + 3), plain)]
for multi in (0, 1):
    t.check_all(L, dd._pkg(), o, ins, multi, streaming=False)
print("ok")
"""


def test_batch_forms_in_shrunk_groups():
    """the same through several groups and the oversized-input path of both batch forms (the group size is read once per process)"""
    env = dict(os.environ, CJS_DEBUG="1", CJS_DEC_GROUP_BYTES="200000")
    r = subprocess.run([sys.executable, "-c", _SHRUNK], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().endswith("ok"), r.stdout[-2000:]
    groups = [l for l in r.stderr.splitlines() if l.startswith("[cjs dec batch] group:")]
    units = [int(l.split(" units")[0].split()[-1]) for l in r.stderr.splitlines() if l.startswith("[cjs dec dev] batch:")]
    assert len(groups) >= 2 * 3 and len(units) == 2 and all(u >= 5 for u in units), (len(groups), units)
