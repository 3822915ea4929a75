"""The host range coder of BWTC compression (HostCoder in csrc/bwtc_host.h: division, reciprocal and two-thread forms of one
arithmetic) against the oracle's coder, byte for byte, on the crafted step lists of tests/bwtc_cases.py, through
cjs_stage_bwtc_code in both modes.  Host logic only: runs without a GPU."""
import numpy as np
import pytest

import bwtc_cases as bc

_WANT = {}


def _want(oracle, c):
    if c["name"] not in _WANT:
        rc, out, _ = oracle.rc_encode_steps(c["first_byte"], c["steps"])
        assert rc == 0
        _WANT[c["name"]] = out
    return _WANT[c["name"]]


@pytest.mark.parametrize("mode", (0, 1), ids=("one-thread", "split"))
@pytest.mark.parametrize("family", ("C1", "C2", "C3", "C4"))
def test_stage_code_equals_oracle(oracle, hip, family, mode):
    assert "cjs_stage_bwtc_code" not in hip.missing
    cases = [c for c in bc.coder_cases() if c["family"] == family]
    assert cases
    for c in cases:
        want = _want(oracle, c)
        rc, got = hip.stage_bwtc_code(c["steps"], c["first_byte"], mode)
        assert rc == 0, c["name"]
        if got.size != want.size or not np.array_equal(got, want):
            n = min(got.size, want.size)
            d = np.nonzero(got[:n] != want[:n])[0]
            at = int(d[0]) if d.size else n
            raise AssertionError("%s (mode %d, %d steps): %d bytes, oracle %d; first difference at byte %d: %s, oracle %s"
                                 % (c["name"], mode, c["steps"].size, got.size, want.size, at,
                                    got[at: at + 6].tobytes().hex(), want[at: at + 6].tobytes().hex()))


def test_stage_code_refuses_invalid_steps(hip):
    for w in (bc.SHIFT | 1 | (0 << 16) | (0 << 32), 0 | (0 << 16) | (5 << 32), 3 | (3 << 16) | (5 << 32),
              bc.SHIFT | 2 | (255 << 16) | (8 << 32), 1 | (0 << 16) | (0 << 32), 1 | (1 << 49) | (3 << 32),
              bc.SHIFT | 1 | (17 << 32)):
        rc, out = hip.stage_bwtc_code(np.array([bc.freq(1, 0, 3), w], dtype=np.uint64), 0x80, 0)
        assert rc == -32 and out is None, hex(w)          # CJS_E_INVALID_ARG
    assert hip.stage_bwtc_code(np.zeros(0, dtype=np.uint64), 0x80, 2)[0] == -32
