"""Inputs of the piece tests (test_gpu_enc_pieces.py): streams of a known number of blocks, every block of another kind than its
neighbours, so that a per-block row read from the wrong block cannot give the oracle's stream.

An input is a sequence of stretches.  Every stretch but the last fills exactly one block (cap bytes after RLE1):

  T  recipes.textgen text                         R  uniform random bytes (256 symbols)
  W  random bytes over two symbols                A  "ab" repeated (many sort rounds)
  Z  300,000 zeros, then text: 5,885 bytes after RLE1, so every block boundary behind it moves by 294,115 input bytes

T, R, W and A hold no run of four equal bytes, so RLE1 leaves them as they are.  The last stretch is text of the length the case
names: 1 byte, exactly cap bytes, or something between.  blocks(oracle, name) is the oracle's word on all of this
(test_enc_pieces_cases_are_what_they_say checks it without a GPU)."""
import os

import numpy as np

import recipes

CAP1, CAP9 = 99981, 899981
ZEROS = 300000
ZEROS_RLE1 = 5 * (ZEROS // 255 + 1)            # 1,176 runs of 255 and one of 120: four bytes and a count each

# name -> (level, kinds of the full blocks, bytes of the last stretch or 0: the last full block ends the input)
CASES = {
    "b1": (1, "", 60000),
    "b2": (1, "RW", 0),
    "b3": (1, "ZR", 1),
    "b4": (1, "TWRA", 0),
    "b5": (1, "ARZW", 30000),
    "b7": (1, "TRWZAR", 1),
    "b9": (1, "ARTWZRWRT", 0),
    "b10": (1, "ARTWZRTWR", 40000),
    "b13": (1, "ATRWZARTWRAR", 12345),
    "l9b5": (9, "TWRA", 100000),
}
NBLOCKS = {"b1": 1, "b2": 2, "b3": 3, "b4": 4, "b5": 5, "b7": 7, "b9": 9, "b10": 10, "b13": 13, "l9b5": 5}
LEVEL1 = ["b1", "b2", "b3", "b4", "b5", "b7", "b9", "b10", "b13"]
ALL = LEVEL1 + ["l9b5"]

_inputs = {}


def _no_runs(a):
    """a with the fourth byte of every run of four equal bytes changed (in place)"""
    while a.size >= 4:
        hit = np.flatnonzero((a[3:] == a[2:-1]) & (a[3:] == a[1:-2]) & (a[3:] == a[:-3])) + 3
        if hit.size == 0:
            break
        a[hit[np.diff(hit, prepend=-8) > 3]] ^= 0x55      # (hits inside a longer run are looked at again)
    return a


def _stretch(kind, n, seed):
    """n bytes of `kind` that RLE1 leaves alone (Z: n bytes after RLE1)"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "T":
        a = _no_runs(recipes.textgen(n, 40 + seed).copy())
    elif kind == "R":
        a = _no_runs(rng.integers(0, 256, n, dtype=np.uint8))
    elif kind == "W":                            # runs of 1..3 of 0xC1 and 0xC2 by turns
        runs = rng.integers(1, 4, n, dtype=np.int64)
        a = np.repeat((np.arange(n) & 1).astype(np.uint8) + 0xC1, runs)[:n].copy()
    elif kind == "A":
        a = np.tile(np.frombuffer(b"ab", np.uint8), n // 2 + 1)[:n].copy()
    elif kind == "Z":
        text = _no_runs(recipes.textgen(n - ZEROS_RLE1, 40 + seed).copy())
        if text[0] == 0:
            text[0] = 0x41
        a = np.concatenate([np.zeros(ZEROS, np.uint8), text])
    else:
        raise KeyError(kind)
    return a


def _part_seam(kind_a, a, kind_b, b):
    """no run across the seam of two stretches: where a's last byte is b's first, one of the two becomes another letter -- a's in
    text and random bytes, whose alphabets are free, else b's (which is text or random then: W and A end in none of Z's zeros)"""
    if a[-1] != b[0]:
        return
    if kind_a in "TRZ":
        a[-1] = next(c for c in b"eta" if c != b[0] and (a.size < 2 or c != a[-2]))
    else:
        assert kind_b in "TR"
        b[0] = next(c for c in b"eto" if c != a[-1] and (b.size < 2 or c != b[1]))


def data(name):
    """the input (read-only, made once)"""
    if name not in _inputs:
        level, kinds, last = CASES[name]
        cap = level * 100000 - 19
        parts = [_stretch(kind, cap, 16 * len(name) + k) for k, kind in enumerate(kinds)]
        if last:
            parts.append(_stretch("T", last, 99 + len(name)))
        kinds = kinds + ("T" if last else "")
        for k in range(1, len(parts)):
            _part_seam(kinds[k - 1], parts[k - 1], kinds[k], parts[k])
        a = np.concatenate(parts)
        a.setflags(write=False)
        _inputs[name] = a
    return _inputs[name]


def level(name):
    return CASES[name][0]


def stretch_bounds(name):
    """input offsets at which the stretches of `name` start, and the input's size behind them"""
    level, kinds, last = CASES[name]
    cap = level * 100000 - 19
    sizes = [cap + (ZEROS - ZEROS_RLE1 if kind == "Z" else 0) for kind in kinds] + ([last] if last else [])
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64).tolist()


def piece_sizes(cnt, split):
    """the blocks of the pieces a call over cnt blocks goes in (csrc/enc_pieces.h): four pieces of ceil(cnt / 4) while blocks are
    left when `split`, else one"""
    if cnt == 0:
        return []
    per = -(-cnt // 4) if split else cnt
    return [min(per, cnt - k0) for k0 in range(0, cnt, per)]


def piece_ranges(cnt, split):
    """(k0, kc) of those pieces"""
    out, k0 = [], 0
    for kc in piece_sizes(cnt, split):
        out.append((k0, kc))
        k0 += kc
    return out


class knob:
    """with knob(True): CJS_ENC_PIECE_BYTES=1 (every call with a tail stream and no stage timers goes in pieces); knob(False): unset
    (the library reads the variable at every call)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.pop("CJS_ENC_PIECE_BYTES", None)
        if self.on:
            os.environ["CJS_ENC_PIECE_BYTES"] = "1"
        return self

    def __exit__(self, *exc):
        os.environ.pop("CJS_ENC_PIECE_BYTES", None)
        if self.old is not None:
            os.environ["CJS_ENC_PIECE_BYTES"] = self.old
        return False
