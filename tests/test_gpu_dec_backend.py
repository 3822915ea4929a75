"""-m gpu: the second half of the Bzip2 decoder -- the inverse BWT (ib_*, csrc/dec_ibwt.hip) and the RLE1 expansion (unrle1_*,
ur_load, csrc/dec_unrle1.hip) -- on blocks built byte by byte (bzblocks.py), against the Python restatement of the reference's two loops.

Family R gives the expansion its borders: count bytes on either side of a thread's 16 bytes, a wave's 1024 and a tile's 16384,
count bytes equal to their run's byte, single-value stretches over one and two tile borders, block ends in the middle of a run,
tiles that expand to just below and above the staging limit, every block offset and output alignment.  Family W gives the walk
stretches between splitters of exactly SEG_CAP - 1 .. SEG_CAP + 1 steps and of tens of thousands, start slots on and off a
splitter, periodic blocks, and `tt` arrays that are no BWT: cycles through the start that do not divide the block length.
test_bzblocks_host.py checks on the CPU that the cases have these properties and that the oracle decodes them the same way."""
import importlib
import sys

import numpy as np
import pytest

import bzblocks as bz
import support

pytestmark = pytest.mark.gpu


def _pkg():
    sys.path.insert(0, support.ROOT)
    return importlib.import_module("compressjs-flattened_amd")


def _same(got, want, what):
    assert bytes(got) == want, (what, bz.first_difference(got, want))


@pytest.mark.parametrize("name", [c.name for c in bz.CASES])
def test_case(hip, oracle, name):
    stream, want = bz.stream(oracle, bz.BY_NAME[name])
    rc, got = hip.bzip2_decompress(stream)
    assert rc == 0, (name, rc, hip.last_error_detail())
    _same(got.tobytes(), want, name)


@pytest.mark.parametrize("name", [c.name for c in bz.SENTINEL_CASES])
def test_sentinel_form(hip, oracle, name):
    # W5: the same bytes as one BWTC block: ib_pack_sentinel and the sentinel branches of both walks
    w = bz.BY_NAME[name].make()[1][0]
    rc, packed = oracle.bwtc_compress(w, 9)
    assert rc == 0
    rc, got = hip.bwtc_decompress(packed)
    assert rc == 0, (name, rc, hip.last_error_detail())
    _same(got.tobytes(), w.tobytes(), name)


def test_all_streams_in_one_host_batch(oracle):
    # cjs_bzip2_decompress_batch: every stream's blocks back to back in shared passes
    built = [bz.stream(oracle, c) for c in bz.CASES]
    outs = _pkg().Bzip2.decompressFiles([s for s, _ in built])
    assert len(outs) == len(built)
    for case, (_, want), got in zip(bz.CASES, built, outs):
        _same(got.tobytes(), want, case.name)


def test_all_streams_in_one_device_batch(oracle):
    import torch
    built = [bz.stream(oracle, c) for c in bz.CASES]
    offs = np.concatenate([[0], np.cumsum([s.size for s, _ in built])]).astype(np.uint64)
    d_in = torch.from_numpy(np.concatenate([s for s, _ in built] + [np.zeros(1, np.uint8)])).cuda()
    total = sum(len(want) for _, want in built)
    d_out = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    off, ln, status, detail = _pkg().decompress_batch_device(d_in.data_ptr(), offs, d_out.data_ptr(), total)
    assert not status.any(), (status.nonzero()[0][:5], detail)
    host = d_out.cpu().numpy()
    assert bool((host[total:] == 0xA5).all())
    for k, (case, (_, want)) in enumerate(zip(bz.CASES, built)):
        assert int(ln[k]) == len(want), (case.name, int(ln[k]), len(want))
        _same(host[int(off[k]): int(off[k]) + int(ln[k])].tobytes(), want, case.name)


def test_six_streams_on_the_device_one_by_one(oracle):
    import torch
    pkg = _pkg()
    for name in ("R5-maximal", "R2-v255-n50000-lead3", "R6-17-blocks", "W1-page384-x64-low1", "W3-p2-n20000", "W4-n100000-of3-orig99999"):
        stream, want = bz.stream(oracle, bz.BY_NAME[name])
        d_in = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), stream, np.zeros(1, np.uint8)])).cuda()
        d_out = torch.full((len(want) + 5 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        n = pkg.decompress_device(d_in.data_ptr() + 3, stream.size, d_out.data_ptr() + 5, len(want))
        host = d_out.cpu().numpy()
        assert n == len(want), (name, n, len(want))
        _same(host[5: 5 + n].tobytes(), want, name)
        assert bool((host[:5] == 0xA5).all()) and bool((host[5 + n:] == 0xA5).all()), name
