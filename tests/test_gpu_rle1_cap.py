"""Stage 0 (RLE1, block boundaries, block CRCs) against the oracle with the block capacity as a free argument
(cjs_stage_rle1_cap): thousands of block boundaries at every chunk phase in inputs of a few tiles, the rounds of the boundary walk,
the materialise kernel's two paths, the chunk seam of the tile scans, rle1_finish by windows on a used workspace, and the tile
tables made share by share.  tests/rle1_cases.py builds the families; tests/test_rle1_cases_host.py shows on the CPU that each
contains what it says.  Every field is compared exactly: nblocks, last_len, and per block s, e, len, the bytes and the crc."""
import numpy as np
import pytest

import rle1_cases as rc

pytestmark = pytest.mark.gpu

INVALID_ARG = -32


def compare(got, last, want, what):
    assert len(got) == len(want), "%s: %d blocks, want %d" % (what, len(got), len(want))
    assert last == (want[-1][0].size if want else 0), "%s: last_len %d" % (what, last)
    flat = lambda bl: np.concatenate([b[0] for b in bl] + [np.zeros(0, np.uint8)])
    if [(b[0].size,) + b[1:] for b in got] == [(b[0].size,) + b[1:] for b in want] and np.array_equal(flat(got), flat(want)):
        return                                               # all equal; else say where
    for k, ((gb, gcrc, gs, ge), (wb, wcrc, ws, we)) in enumerate(zip(got, want)):
        assert (gs, ge) == (ws, we), "%s: block %d input [%d, %d), want [%d, %d)" % (what, k, gs, ge, ws, we)
        assert gb.size == wb.size, "%s: block %d len %d want %d" % (what, k, gb.size, wb.size)
        if not np.array_equal(gb, wb):
            bad = np.nonzero(gb != wb)[0]
            raise AssertionError("%s: block %d [%d, %d): %d bytes differ, first at %d (got %d want %d)"
                                 % (what, k, gs, ge, bad.size, bad[0], gb[bad[0]], wb[bad[0]]))
        assert gcrc == wcrc, "%s: block %d crc %08x want %08x" % (what, k, gcrc, wcrc)


def check(hip, oracle, key, data, cap, world=1, range_blocks=0, work_fill=0):
    what = "%s cap %d world %d range_blocks %d fill %02x" % (key, cap, world, range_blocks, work_fill)
    rc_, got, last = hip.stage_rle1_cap(data, cap, world, range_blocks, work_fill)
    assert rc_ == 0, "%s: rc %d" % (what, rc_)
    compare(got, last, rc.want(oracle, key, data, cap), what)
    return got


def test_family_a_boundary_phases(hip, oracle):
    for name, cap in rc.family_a():
        check(hip, oracle, name, rc.inputs()[name], cap)


def test_family_b_speculation_rounds(hip, oracle):
    for name, (data, cap) in sorted(rc.family_b().items()):
        for world in (1, 2):
            check(hip, oracle, "b_" + name, data, cap, world)


def test_family_c_geometry(hip, oracle):
    for name, (data, cap) in sorted(rc.family_c(oracle.rle1_len).items()):
        check(hip, oracle, "c_offsets" if name.startswith("offsets_") else "c_" + name, data, cap)


@pytest.mark.parametrize("L", rc.C_SEAM_RUNS)
def test_family_c_chunk_seam(hip, oracle, L):
    check(hip, oracle, "c_seam_%d" % L, rc.chunk_seam_input(L), rc.C_SEAM_CAP)


def test_family_d_fast_path(hip, oracle):
    for name, cap in rc.family_d():
        check(hip, oracle, name, rc.inputs()[name], cap, work_fill=0xFF)


def test_family_e_ranged_finish(hip, oracle):
    for name, cap in rc.family_e():
        data = rc.inputs()[name]
        whole = check(hip, oracle, name, data, cap)
        for rb in rc.E_RANGES:
            for fill in rc.E_FILLS:
                got = check(hip, oracle, name, data, cap, 1, rb, fill)
                assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(got, whole))


def test_family_f_shares(hip, oracle):
    for name, (data, caps) in sorted(rc.family_f().items()):
        for cap in caps:
            one = check(hip, oracle, name, data, cap)
            for world in rc.F_WORLDS:
                got = check(hip, oracle, name, data, cap, world, 0, 0xFF)
                assert all(np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(got, one))


def test_family_h_sweep(hip, oracle):
    for i, data, cap in rc.family_h():
        for world in (1, 2):
            try:
                check(hip, oracle, "h/%d" % i, data, cap, world, 0, 0xFF if i & 1 else 0)
            except AssertionError as e:
                raise AssertionError("(seed %d, index %d, cap %d): %s" % (rc.H_SEED, i, cap, e))


def test_refusals(hip):
    data = rc.noise(100)
    for cap in (0, 1, rc.CAP_FLOOR - 1, 899982):
        assert hip.stage_rle1_cap(data, cap)[0] == INVALID_ARG, cap
    assert hip.stage_rle1_cap(data, 50, world=0)[0] == INVALID_ARG
    assert hip.stage_rle1_cap(data, rc.CAP_FLOOR)[0] == 0
    assert hip.stage_rle1_cap(data, 899981)[0] == 0
    rc_, got, last = hip.stage_rle1_cap(np.zeros(0, np.uint8), 50, 3, 2, 0xFF)
    assert rc_ == 0 and got == [] and last == 0
