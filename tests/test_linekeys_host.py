"""The host side of the line keys, without a GPU: cjs_stage_line_keys (csrc/line_key.h over a plain buffer) against the key restated
with Python's big integers, and cjs_line_keys_diff (csrc/line_diff.h) by property against the quadratic DP."""
import ctypes

import numpy as np
import pytest

import linekeys_cases as lk
import range_cases as rg

SEEDS = (0, 0x0123456789ABCDEF)


@pytest.fixture(scope="module")
def L():
    return lk.bind()


def _texts():
    rng = np.random.RandomState(99)
    words = [bytes(rng.randint(32, 127, int(rng.randint(0, 40))).astype(np.uint8)) for _ in range(50)]
    text = b"\n".join(words[int(i)] for i in rng.randint(0, 50, 400))
    binary = bytes(rng.choice(np.array([0, 0xFF, 10, 0x0B, 0x8A, 65], np.uint8), 5000))
    return {"text, no final newline": text, "text, final newline": text + b"\n", "binary": binary, "empty": b"", "newline": b"\n",
            "newlines": b"\n\n\n", "one byte": b"\0", "long line": bytes(rng.randint(0, 256, 70000).astype(np.uint8)).replace(b"\n", b"\r")}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", sorted(_texts()))
def test_stage_keys_against_the_restatement(L, name, seed):
    text = _texts()[name]
    want = lk.text_keys(text, seed)
    rc, keys, n = lk.stage_keys(L, text, seed)
    assert rc == 0 and n == len(want) == text.count(b"\n") + 1
    assert lk.as_tuples(keys) == want
    assert all(h < lk.P for h, _, _ in want)
    if name == "text, final newline":
        assert want[-1] == (0, 0, 0)                        # the tail line is empty


def test_the_restatement_is_the_issues_formula():
    b1, b2 = lk.bases(5)
    assert 256 <= b1 < lk.P and 256 <= b2 < lk.P and b1 != b2 and lk.bases(6) != (b1, b2)
    line = b"ab\n"
    assert lk.line_key(line, b1, b2) == ((98 * b1 * b1 + 99 * b1 + 11) % lk.P, 3, ((98 * b2 * b2 + 99 * b2 + 11) % lk.P) & 0xFFFFFFFF)


def test_zero_bytes_move_the_hash(L):
    got = [lk.as_tuples(lk.stage_keys(L, t, 0)[1])[0] for t in (b"", b"\0", b"\0\0")]
    assert len({g[0] for g in got}) == 3 and len({g[2] for g in got}) == 3 and [g[1] for g in got] == [0, 1, 2]


def test_seeds_give_different_keys(L):
    a, b = (lk.as_tuples(lk.stage_keys(L, b"some line\n", s)[1]) for s in SEEDS)
    assert a[0][0] != b[0][0] and a[0][2] != b[0][2] and a[0][1] == b[0][1] == 10


def test_stage_keys_cap(L):
    text = _texts()["text, no final newline"]
    want = lk.text_keys(text, 3)
    for cap in (0, 1, 7, len(want) - 1, len(want) + 5):
        rc, keys, n = lk.stage_keys(L, text, 3, cap)          # (stage_keys checks that nothing past min(cap, n) is written)
        assert rc == 0 and n == len(want) and lk.as_tuples(keys) == want[:cap]


def test_stage_keys_argument_errors(L):
    n = rg.S(0)
    k = np.zeros(4, dtype=lk.KEY)
    assert L.cjs_stage_line_keys(None, 3, 0, k.ctypes.data, 4, ctypes.byref(n)) == rg.E_INVALID
    assert L.cjs_stage_line_keys(b"abc", 3, 0, None, 4, ctypes.byref(n)) == rg.E_INVALID
    assert L.cjs_stage_line_keys(b"abc", 3, 0, k.ctypes.data, 4, None) == rg.E_INVALID
    assert L.cjs_stage_line_keys(None, 0, 0, None, 0, ctypes.byref(n)) == 0 and n.value == 1


# ---------------------------------------------------------------- the diff
def _pool():
    b1, b2 = lk.bases(1)
    return [lk.line_key(b"line %d\n" % k, b1, b2) for k in range(12)]


def _pairs():
    rng = np.random.RandomState(2024)
    pool = _pool()
    out = []
    for i in range(500):
        small = pool[:int(rng.randint(2, 13))]
        na, nb = (int(rng.randint(0, 301)) for _ in range(2))
        a = [small[int(k)] for k in rng.randint(0, len(small), na)]
        if i % 3 == 0:                                      # B is A with a few edits: long common stretches
            b = list(a)
            for _ in range(int(rng.randint(0, 12))):
                p = int(rng.randint(0, len(b) + 1))
                if rng.randint(0, 2) and b:
                    del b[min(p, len(b) - 1)]
                else:
                    b.insert(p, small[int(rng.randint(0, len(small)))])
        else:
            b = [small[int(k)] for k in rng.randint(0, len(small), nb)]
        out.append((a, b))
    return out


def test_diff_on_random_pairs(L):
    for a, b in _pairs():
        rc, hunks, info = lk.diff(L, a, b)
        assert rc == 0 and info.minimal == 1
        lk.check_hunks(a, b, hunks, info)
        assert info.edits == lk.edit_distance(a, b), (len(a), len(b))


def test_diff_fixed_cases(L):
    p = _pool()
    a = p[:8]
    for x, y, want in ((a, a, []), ([], [], []), (a, [], [(0, 8, 0, 0)]), ([], a, [(0, 0, 0, 8)]),
                       (a, p[8:10] + a[2:], [(0, 2, 0, 2)]), (a, a[:6] + p[9:12], [(6, 2, 6, 3)]), (a, a[:3] + a[4:], [(3, 1, 3, 0)]),
                       (a, a[:3] + [p[9]] + a[3:], [(3, 0, 3, 1)]), (p[:4], p[4:9], [(0, 4, 0, 5)]), ([p[0]], [p[1]], [(0, 1, 0, 1)]),
                       (a, [a[0]] + p[8:10] + a[3:5] + a[6:], [(1, 2, 1, 2), (5, 1, 5, 0)])):
        rc, hunks, info = lk.diff(L, x, y)
        assert rc == 0 and hunks == want and info.minimal == 1, (hunks, want)
        lk.check_hunks(x, y, hunks, info)
    rc, hunks, info = lk.diff(L, a, a)
    assert info.edits == 0 and info.common == 8 and info.n_hunks == 0


def test_all_ones_records_equal_nothing(L):
    p = _pool()
    a = [p[0], lk.ONES, p[1]]
    rc, hunks, info = lk.diff(L, a, a)
    assert rc == 0 and hunks == [(1, 1, 1, 1)] and info.edits == 2 and info.common == 2


def test_max_edits_below_the_minimum(L):
    rng = np.random.RandomState(8)
    p = _pool()
    a = [p[int(k)] for k in rng.randint(0, 12, 200)]
    b = [p[int(k)] for k in rng.randint(0, 12, 180)]
    a, b = [p[3]] * 5 + a + [p[4]] * 7, [p[3]] * 5 + b + [p[4]] * 7      # a common prefix and suffix around the middle
    least = lk.edit_distance(a, b)
    assert least > 40
    for cap_edits, minimal in ((least, 1), (least + 1, 1), (least - 1, 0), (1, 0), (10 ** 9, 1)):
        rc, hunks, info = lk.diff(L, a, b, cap_edits)
        assert rc == 0 and info.minimal == minimal, (cap_edits, least, info.edits)
        lk.check_hunks(a, b, hunks, info)
        if minimal:
            assert info.edits == least
        else:                                               # everything between the common prefix and suffix is one hunk
            assert len(hunks) == 1 and hunks[0][0] == hunks[0][2] and hunks[0][0] >= 5 and hunks[0][0] + hunks[0][1] <= len(a) - 7
            assert lk.diff(L, a, b, cap_edits)[1] == hunks   # deterministic
    rc, hunks, info = lk.diff(L, a, b)                       # 0 is the default, far above this minimum
    assert info.minimal == 1 and info.edits == least


def test_cap_below_the_hunks(L):
    a, b = next((a, b) for a, b in _pairs() if lk.diff(L, a, b)[2].n_hunks >= 5)
    rc, full, info = lk.diff(L, a, b)
    for cap in (0, 1, 3, len(full) - 1, len(full) + 4):
        rc, hunks, info2 = lk.diff(L, a, b, cap=cap)         # (diff checks that nothing past min(cap, n_hunks) is written)
        assert rc == 0 and hunks == full[:cap] and info2.n_hunks == len(full) and info2.edits == info.edits


def test_diff_argument_errors(L):
    k = lk.key_array(_pool())
    info = lk.DiffInfo()
    h = np.zeros(4, dtype=lk.HUNK)
    assert L.cjs_line_keys_diff(k.ctypes.data, 3, k.ctypes.data, 3, 0, h.ctypes.data, 4, None) == rg.E_INVALID
    assert L.cjs_line_keys_diff(None, 3, k.ctypes.data, 3, 0, h.ctypes.data, 4, ctypes.byref(info)) == rg.E_INVALID
    assert L.cjs_line_keys_diff(k.ctypes.data, 3, None, 3, 0, h.ctypes.data, 4, ctypes.byref(info)) == rg.E_INVALID
    assert L.cjs_line_keys_diff(k.ctypes.data, 3, k.ctypes.data, 3, 0, None, 4, ctypes.byref(info)) == rg.E_INVALID
    assert L.cjs_line_keys_diff(None, 0, None, 0, 0, None, 0, ctypes.byref(info)) == 0 and info.n_hunks == 0 and info.minimal == 1
