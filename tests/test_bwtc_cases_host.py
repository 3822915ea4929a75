"""Every crafted case of tests/bwtc_cases.py reaches the state it was made for: asserted from the oracle's event counters (model
blocks) and from the coder statistics of rc_encode_steps (step lists).  A case that misses its state is a broken test.  CPU only."""
import numpy as np
import pytest

import bwtc_cases as bc


@pytest.mark.parametrize("family", bc.M_FAMILIES + bc.D_FAMILIES)
def test_model_cases_reach_their_state(oracle, family):
    cases = bc.model_cases(family)
    assert cases
    nchecks = 0
    for c in cases:
        assert c["A"].size <= 4096 and c["A"].dtype == np.uint16 and 1 <= c["asz"] <= 256
        assert c["A"].size == 0 or int(c["A"].max()) <= c["asz"], c["name"]
        assert c["fast"] == (family[0] == "D")
        for upto, event, op, value in c["checks"]:
            got = oracle.bwtc_model_steps(c["A"][:upto], c["asz"], c["fast"])[2][event]
            assert (got == value) if op == "eq" else (got >= value), \
                "%s: %s over A[:%s] is %d, the case needs %s %d" % (c["name"], event, upto, got, op, value)
            nchecks += 1
    if family not in ("M1", "D1"):
        assert nchecks >= len(cases), "every case of %s names a state" % family


def test_grid_covers_the_alphabet_seams(oracle):
    # ns = asz + 2 on and beside every power of two; r0 == 0 exactly on them; the largest alphabet; "high" stays off symbols < r0
    assert {a + 2 for a in bc.M1_ASZ} >= {4, 8, 16, 32, 64, 128, 256, 258} | {3, 5, 9, 16 + 1, 33, 65, 129, 257}
    assert {bc.r0_of(a) == 0 for a in bc.M1_ASZ} == {True, False}
    for a in bc.M1_ASZ:
        ns = a + 2
        assert (bc.r0_of(a) == 0) == (ns & (ns - 1) == 0) and 0 <= bc.r0_of(a) < ns
    lens = set()
    for c in bc.model_cases("M1"):
        lens.add(c["A"].size)
        if "-high-" in c["name"]:
            assert int(c["A"].min()) >= bc.r0_of(c["asz"])
    assert lens == set(bc.M1_LEN)
    # the grid as a whole meets the model's common states many times over
    tot = {}
    for c in bc.model_cases("M1"):
        for k, v in oracle.bwtc_model_steps(c["A"], c["asz"], False)[2].items():
            tot[k] = tot.get(k, 0) + v
    assert tot["rescale"] > 1000 and tot["escape"] > 1000 and tot["last_escape"] > 50, tot


def test_m2_last_escape_falls_on_every_lane():
    # position of the last first-occurrence inside its 64-symbol chunk, over the family
    lanes = set()
    for c in bc.model_cases("M2"):
        _, first = np.unique(c["A"], return_index=True)
        lanes.add(int(first.max()) % 64)
    assert lanes == set(range(64))


@pytest.mark.parametrize("family", ("C1", "C2", "C3", "C4"))
def test_coder_cases_reach_their_state(oracle, family):
    cases = [c for c in bc.coder_cases() if c["family"] == family]
    assert cases
    seen_shifts = set()
    for c in cases:
        rc, out, st = oracle.rc_encode_steps(c["first_byte"], c["steps"])
        assert rc == 0, c["name"]
        seen_shifts.add(st["max_shifts"])
        for k, v in c["expect"].items():
            if k == "min_help":
                assert v <= st["max_help"] <= v + 8, "%s: %s" % (c["name"], st)
            elif k == "max_shifts":
                assert st["max_shifts"] == v, "%s: %s" % (c["name"], st)
            else:
                assert st[k] == v, "%s: %s, wanted %s == %d" % (c["name"], st, k, v)
    if family == "C1":
        runs = {c["expect"]["min_help"] for c in cases}
        assert runs == set(bc.C1_RUNS)
        assert sum(c["expect"]["carries"] for c in cases) == 2 * len(bc.C1_RUNS)
    if family == "C2":
        assert {2, 3} <= seen_shifts
    if family == "C3":
        assert sorted({c["steps"].size for c in cases}) == sorted(bc.C3_LEN)
