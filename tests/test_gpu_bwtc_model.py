"""The model kernels of BWTC compression (bwtc_fenwick_par for levels 6..9, bwtc_defsum for levels 1..5) against the oracle's
models step by step, on the crafted blocks of tests/bwtc_cases.py: same number of steps, same 64-bit words.  One launch per
family and level (cjs_stage_bwtc_model takes many blocks).  The kernel depends on the family only, so levels 6 and 1 carry every
case and levels 9 and 5 a thin slice.  Plus one end-to-end check of the two stage hooks together."""
import numpy as np
import pytest

import bwtc_cases as bc

pytestmark = pytest.mark.gpu

_WANT = {}


def _want(oracle, family):
    """the oracle's (steps, symbol position of each step) of every case of a family, computed once"""
    if family not in _WANT:
        _WANT[family] = [oracle.bwtc_model_steps(c["A"], c["asz"], c["fast"])[:2] for c in bc.model_cases(family)]
    return _WANT[family]


def _unpack(w):
    w = int(w)
    return "%s(sy=%d, lt=%d, %s=%d)" % ("shift" if w >> 63 else "freq", w & 0xFFFF, (w >> 16) & 0xFFFF,
                                       "shift" if w >> 63 else "tot", (w >> 32) & 0x1FFFF)


def _compare(c, got, want, pos, level):
    if got is not None and got.size == want.size and np.array_equal(got, want):
        return
    if got is None:
        raise AssertionError("%s (family %s, asz %d, level %d): the kernel reports more steps than two per symbol"
                             % (c["name"], c["family"], c["asz"], level))
    n = min(got.size, want.size)
    d = np.nonzero(got[:n] != want[:n])[0]
    at = int(d[0]) if d.size else n
    sym_at = int(pos[min(at, pos.size - 1)]) if pos.size else 0
    raise AssertionError("%s (family %s, asz %d, level %d): %d steps, oracle %d; first differing step %d, of symbol position %d "
                         "(symbol %d): %s, oracle %s"
                         % (c["name"], c["family"], c["asz"], level, got.size, want.size, at, sym_at,
                            int(c["A"][sym_at]) if c["A"].size else -1, _unpack(got[at]) if at < got.size else "nothing",
                            _unpack(want[at]) if at < want.size else "nothing"))


CASES = [(f, 6, 1) for f in bc.M_FAMILIES] + [("M1", 9, 5), ("M2", 9, 97), ("M3", 9, 3), ("M4", 9, 2), ("M5", 9, 1)] + \
        [(f, 1, 1) for f in bc.D_FAMILIES] + [("D1", 5, 5), ("D2", 5, 2), ("D3", 5, 2), ("D4", 5, 1)]


@pytest.mark.parametrize("family,level,every", CASES, ids=["%s-level%d" % (f, lv) for f, lv, _ in CASES])
def test_model_steps_equal_oracle(oracle, hip, family, level, every):
    cases = bc.model_cases(family)[::every]
    want = _want(oracle, family)[::every]
    rc, got = hip.stage_bwtc_model([(c["A"], c["asz"]) for c in cases], level)
    assert rc == 0
    for c, g, (w, pos) in zip(cases, got, want):
        _compare(c, g, w, pos, level)


@pytest.mark.parametrize("name,level", [("sample3", 1), ("sample3", 9), ("long_runs_mixed", 6)])
def test_model_and_coder_hooks_make_the_stream(oracle, hip, name, level):
    # the product's model steps of every block, spliced between the oracle's framing steps, through the product's coder
    data = bc.golden_input(name)
    rc, steps, prefix_n, first_byte, blocks = oracle.bwtc_stream_steps(data, level)
    assert rc == 0 and blocks
    bs = level * 100000
    syms = []
    for k in range(len(blocks)):
        U, _ = oracle.bwt_sentinel(data[k * bs: (k + 1) * bs])
        A, _, asz = oracle.mtf_rle2(U, U)
        syms.append((A[:-1], asz))                    # (bzip2's end-of-block symbol is not part of BWTC's stream)
    rc, got = hip.stage_bwtc_model(syms, level)
    assert rc == 0
    parts, at = [], 0
    for (lo, hi), g in zip(blocks, got):
        assert g is not None and np.array_equal(g, steps[lo:hi]), "block model steps differ"
        parts += [steps[at:lo], g]
        at = hi
    parts.append(steps[at:])
    spliced = np.concatenate(parts)
    rc, want = oracle.bwtc_compress(data, level)
    assert rc == 0
    for mode in (0, 1):
        rc, out = hip.stage_bwtc_code(spliced, first_byte, mode)
        assert rc == 0 and np.array_equal(out, want[prefix_n:]), "mode %d" % mode
