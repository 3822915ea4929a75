"""Crafted inputs for the back half of BWTC compression: symbol blocks for the two model kernels (bwtc_fenwick_par, levels 6..9;
bwtc_defsum, levels 1..5) and step lists for the host range coder.  Built from seeds, without a GPU; pad lengths that are easier
to search than to derive are searched with the oracle while the cases are built.  tests/test_bwtc_cases_host.py asserts from the
oracle's event counters and traces that every case reaches the state it names.

A model case is a dict: family, name, asz (byte values of the block; symbols are 0..asz), A (uint16 symbols), fast (DefSum), and
checks: a list of (upto, event, op, value) read as "the oracle's counter `event` over A[:upto] (None = all of A) is op value".

Fenwick families
  M1  alphabet seams: ns = asz + 2 on and beside every power of two (r0 == 0 and r0 > 0, up to ns = 258), three seeded sequences
      (uniform, geometric towards low symbols, none below r0: symbols on both sides of the escape slot), lengths around the
      64-symbol chunk, the eight-wave round and their multiples.
  M2  every symbol first seen inside one chunk: the last escape falls in the parallel window behind asz earlier escapes; shifted
      by 0..63 leading symbols so that it falls on every lane and across a chunk border.
  M3  a novel symbol on the rescale step: the total reaches F_MAX after coder step 254 (0x100 * (1 + 254) = 0xFF00), so with T
      steps in front of the pair (escape, symbol) T = 253 puts the rescale between the two; the same at the second and third
      rescale.  When the novel symbol is the LAST unseen one its escape step takes the escape count out of the total, so no
      rescale can follow that step: those cases target the last escape next to a rescale, not the counter "between".
  M4  decay and return: a symbol seen once holds 0x100 = 2^8, which NINE halvings take to zero (eight leave 1), so the rescale
      that sets it back to "unseen" is the ninth; cases with 6..10 rescales in between.  A variant sees all symbols first: the
      rescales zero the escape leaf, the decay reinstates it.
  M5  runs: one symbol 4096 times, two alternating, asz = 1 with 0/1 only.
DefSum families
  D1  the M1 grid.
  D2  42..257 distinct symbols first: the 41st escape update is refused by the cap of 40 before the first fold.
  D3  an escape with update_count at thresh - 2, thresh - 1 and just behind the fold, in the second and the third fold period
      (before the first fold every symbol is coded through the escape, so 40 escape updates are pending long before
      update_count nears the threshold: the cap answers first and the threshold refusal cannot be reached there).
  D4  a symbol whose share halves to zero across two folds and is escaped again.
Coder step lists
  C1  runs of pending 0xFF bytes of given lengths, ended by a carry, by a step without one, and by finish's own carry.  A run
      that can still end in a carry needs the carry boundary strictly inside the coder's interval at every step; a fixed step
      cannot hold it there (the distance grows 256-fold per byte), so each step's lt is chosen by simulating the coder.  The runs
      of literal shift(1, 255, 8) steps (interval top exactly on the boundary: no carry possible) are kept beside them.
  C2  two and three byte shifts in one step, totals 1 and 2, lt + sy == tot.
  C3  random valid steps, lengths around the ring buffer fill (32768 records; finish adds one).
  C4  recorded step lists of three small golden inputs.
"""
import numpy as np

import recipes
import support

SHIFT = 1 << 63
F_MAX, F_INC = 0xFF00, 0x100

M1_ASZ = (1, 2, 3, 6, 7, 14, 15, 30, 31, 62, 63, 126, 127, 254, 255, 256)
M1_LEN = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 1024, 4096)

_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        _ORACLE = support.Oracle()
    return _ORACLE


def r0_of(asz):
    """symbols >= r0 sit on the deepest level of the reference's tree (first in cumulative order); ns a power of two: 0"""
    ns = asz + 2
    dpt = (2 * ns - 1).bit_length() - 1
    return (1 << dpt) - ns


def _case(family, name, asz, A, fast, checks=()):
    A = np.asarray(A, dtype=np.uint16)
    assert A.size <= 4096 and (A.size == 0 or int(A.max()) <= asz)
    return {"family": family, "name": name, "asz": asz, "A": A, "fast": fast, "checks": list(checks)}


def _events(A, asz, fast):
    return oracle().bwtc_model_steps(np.asarray(A, dtype=np.uint16), asz, fast)[2]


def _first_len(make, event, want, lo, hi, asz, fast):
    """smallest n in [lo, hi] for which the oracle counts event >= want over make(n) (the counter is monotone in n)"""
    assert _events(make(hi), asz, fast)[event] >= want
    while lo < hi:
        mid = (lo + hi) // 2
        if _events(make(mid), asz, fast)[event] >= want:
            hi = mid
        else:
            lo = mid + 1
    return lo


# ---------------------------------------------------------------------------------------------------------------- M1 / D1
def _grid(family, fast):
    out = []
    for asz in M1_ASZ:
        r0 = r0_of(asz)
        for kind in ("uniform", "geometric", "high"):
            rng = np.random.RandomState(1000 * asz + {"uniform": 1, "geometric": 2, "high": 3}[kind])
            full = {"uniform": lambda n: rng.randint(0, asz + 1, n),
                    "geometric": lambda n: np.minimum(rng.geometric(0.25, n) - 1, asz),
                    "high": lambda n: rng.randint(r0, asz + 1, n)}[kind](4096)
            for n in M1_LEN:
                out.append(_case(family, "%s-asz%d-%s-n%d" % (family, asz, kind, n), asz, full[:n], fast))
    return out


# ---------------------------------------------------------------------------------------------------------------- M2
def _m2():
    out = []
    for asz in range(1, 64):
        rng = np.random.RandomState(7000 + asz)
        syms = np.arange(asz + 1)
        orders = [("asc", syms), ("desc", syms[::-1])] + [("shuf%d" % k, rng.permutation(syms)) for k in range(3)]
        for oname, order in orders:
            body = np.concatenate([order, np.resize(order, 70)])
            for lead in range(64):
                A = np.concatenate([np.zeros(lead, dtype=np.int64), body])
                out.append(_case("M2", "M2-asz%d-%s-lead%d" % (asz, oname, lead), asz, A, False,
                                 [(None, "escape", "eq", asz + 1), (None, "last_escape", "eq", 1)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- M3
def _m3():
    out = []
    for m, asz, last in ((1, 200, False), (7, 200, False), (100, 200, False), (1, 1, True), (7, 7, True), (100, 100, True)):
        rng = np.random.RandomState(3000 + 2 * m + last)
        perm = rng.permutation(asz + 1)
        news, novel = perm[:m], perm[m]
        tail = np.concatenate([rng.choice(perm[: m + 1], 40), perm[m + 1: m + 2], rng.choice(perm[: m + 1], 20)])

        def seq(T, with_pair=True, with_tail=True):        # T coder steps, then the pair of the novel symbol
            parts = [news, np.full(T - 2 * m, news[0])]
            if with_pair:
                parts.append([novel])
            if with_pair and with_tail:
                parts.append(tail)
            return np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])

        for k in (1, 2, 3):
            # R = the coder step behind which rescale k happens while only a seen symbol repeats (every step adds F_INC)
            R = 254 if k == 1 else _first_len(lambda T: seq(T, False), "rescale", k, 2 * m, 2 * m + 1200, asz, False)
            assert _events(seq(R, False), asz, False)["rescale"] == k and _events(seq(R - 1, False), asz, False)["rescale"] == k - 1
            for T in (range(250, 257) if k == 1 else (R - 2, R - 1, R)):
                A = seq(T)
                pair_end = T - 2 * m + m + 1
                if last:          # the last unseen symbol: its escape step lowers the total, no rescale can follow that step
                    checks = [(pair_end, "last_escape", "eq", 1), (pair_end, "rescale_between", "eq", 0)]
                else:
                    # T >= R: the rescale comes before the pair; T == R - 1: between its two steps; T == R - 2: right behind it
                    checks = [(pair_end, "rescale_between", "eq", 1 if T == R - 1 else 0),
                              (pair_end, "rescale", "eq", k if T >= R - 2 else k - 1)]
                out.append(_case("M3", "M3-m%d-asz%d-%s-resc%d-T%d" % (m, asz, "last" if last else "more", k, T), asz, A, False, checks))
    return out


# ---------------------------------------------------------------------------------------------------------------- M4
def _m4():
    out = []
    for asz, x, f in ((5, 3, 0), (40, 0, 39), (255, 255, 1)):
        for resc in (6, 7, 8, 9, 10):
            pad = _first_len(lambda n: np.array([x] + [f] * n), "rescale", resc, 1, 4000, asz, False)
            A = np.array([x] + [f] * pad + [x, f, x, x, f])
            decays = resc >= 9                 # 0x100 >> 8 == 1, >> 9 == 0
            out.append(_case("M4", "M4-asz%d-resc%d" % (asz, resc), asz, A, False,
                             [(pad + 1, "rescale", "eq", resc), (pad + 1, "decay", "ge" if decays else "eq", 1 if decays else 0),
                              (pad + 1, "escape", "eq", 2), (pad + 2, "escape", "eq", 3 if decays else 2)]))
    for asz in (1, 2, 6):                       # every symbol seen first: no unseen symbol left, the rescales zero the escape leaf
        first = np.arange(asz + 1)
        for resc in (9, 10):
            pad = _first_len(lambda n: np.concatenate([first, np.full(n, 1)]), "rescale", resc, 1, 4000, asz, False)
            A = np.concatenate([first, np.full(pad, 1), [0, 1, 0, asz, 1]])
            n0 = asz + 1 + pad
            out.append(_case("M4", "M4-allseen-asz%d-resc%d" % (asz, resc), asz, A, False,
                             [(n0, "last_escape", "eq", 1), (n0, "esc_zeroed", "ge", 1), (n0, "decay", "ge", 1),
                              (n0, "esc_reinstated", "ge", 1), (n0, "escape", "eq", asz + 1), (n0 + 1, "escape", "eq", asz + 2)]))
    return out


def _m5():
    return [_case("M5", "M5-one-symbol", 3, np.full(4096, 2), False, [(None, "escape", "eq", 1), (None, "rescale", "ge", 30)]),
            _case("M5", "M5-one-symbol-asz1", 1, np.full(4096, 0), False, [(None, "escape", "eq", 1)]),
            _case("M5", "M5-alternating", 9, np.resize([4, 9], 4096), False, [(None, "escape", "eq", 2)]),
            _case("M5", "M5-binary", 1, np.random.RandomState(55).randint(0, 2, 4096), False, [(None, "last_escape", "eq", 1)]),
            _case("M5", "M5-binary-alternating", 1, np.resize([0, 1], 4095), False, [(None, "last_escape", "eq", 1)])]


# ---------------------------------------------------------------------------------------------------------------- D2..D4
def _d2():
    out = []
    for n in (42, 43, 64, 100, 200, 257):
        for k in range(3):
            rng = np.random.RandomState(2000 + 10 * n + k)
            perm = rng.permutation(n)
            A = np.concatenate([perm, rng.choice(perm, 50)])
            out.append(_case("D2", "D2-n%d-perm%d" % (n, k), n - 1, A, True,
                             [(41, "refused_cap", "eq", 1), (41, "fold", "eq", 0), (40, "refused_cap", "eq", 0)]))
    return out


def _d3():
    out = []
    for asz, seen, novel in ((20, (0, 1, 2, 3, 4, 5), (10, 11, 12)), (256, (256, 0, 100), (255, 1, 7))):
        rng = np.random.RandomState(4000 + asz)
        prefix = np.resize(seen, _first_len(lambda n: np.resize(seen, n), "fold", 1, 1, 400, asz, True))      # ends on the first fold
        for period in (2, 3):
            def seq(r, with_novel=True):
                return np.concatenate([prefix, np.full(r, seen[0]), [novel[period - 2]] if with_novel else []]).astype(np.int64)
            # r_fold repeats of a seen symbol reach the fold of this period; the refusal needs update_count == thresh - 1
            r_fold = _first_len(lambda r: seq(r, False), "fold", period, 1, 600, asz, True)
            for r, refused, folds in ((r_fold - 2, 0, period), (r_fold - 1, 1, period), (r_fold, 0, period)):
                A = np.concatenate([seq(r), rng.choice(seen, 30), [novel[2]], rng.choice(seen, 10)])
                n0 = prefix.size + r + 1
                out.append(_case("D3", "D3-asz%d-period%d-r%d" % (asz, period, r), asz, A, True,
                                 [(n0, "refused_thresh", "eq", refused), (n0, "fold", "eq", folds), (n0 - 1, "refused_thresh", "eq", 0)]))
            prefix = seq(r_fold, False)                          # ends on this period's fold
    return out


def _d4():
    out = []
    for asz, x, fill in ((10, 7, (0, 1, 2)), (256, 256, (3, 200)), (1, 1, (0,))):
        def seq(n):
            return np.concatenate([[x], np.resize(fill, n)]).astype(np.int64)
        n1 = _first_len(seq, "fold", 1, 1, 600, asz, True)       # 1 + n1 symbols end on the first fold: every one of them escaped
        n2 = _first_len(seq, "fold", 2, n1, 1200, asz, True)
        A = np.concatenate([seq(n2), [x, fill[0], x]])
        out.append(_case("D4", "D4-asz%d" % asz, asz, A, True,
                         [(1 + n1, "escape", "eq", 1 + n1), (1 + n2, "escape", "eq", 1 + n1), (1 + n2, "fold", "eq", 2),
                          (2 + n2, "escape", "eq", 2 + n1)]))
    return out


_MODEL = {}


def model_cases(family):
    if family not in _MODEL:
        _MODEL[family] = {"M1": lambda: _grid("M1", False), "M2": _m2, "M3": _m3, "M4": _m4, "M5": _m5,
                          "D1": lambda: _grid("D1", True), "D2": _d2, "D3": _d3, "D4": _d4}[family]()
    return _MODEL[family]


M_FAMILIES = ("M1", "M2", "M3", "M4", "M5")
D_FAMILIES = ("D1", "D2", "D3", "D4")


# ---------------------------------------------------------------------------------------------------------------- coder steps
def freq(sy, lt, tot):
    assert 1 <= sy and lt + sy <= tot < (1 << 17) and sy < (1 << 16) and lt < (1 << 16)
    return sy | (lt << 16) | (tot << 32)


def shift(sy, lt, sh):
    assert 1 <= sy and lt + sy <= (1 << sh) and 1 <= sh <= 16 and sy < (1 << 16) and lt < (1 << 16)
    return SHIFT | sy | (lt << 16) | (sh << 32)


class _Sim:
    """the encoder's interval (J/BWTC:40-153) followed step by step, to CHOOSE steps; what a list does is read from the oracle"""

    def __init__(self):
        self.low, self.range, self.help = 0, 1 << 31, 0

    def copy(self):
        c = _Sim()
        c.low, c.range, c.help = self.low, self.range, self.help
        return c

    def normalize(self):
        while self.range <= (1 << 23):
            if self.low < (0xFF << 23) or self.low & (1 << 31):
                self.help = 0
            else:
                self.help += 1
            self.low = (self.low << 8) & 0x7FFFFFFF
            self.range <<= 8

    def step(self, w):
        self.normalize()
        sy, lt, tot = w & 0xFFFF, (w >> 16) & 0xFFFF, (w >> 32) & 0x1FFFF
        if w & SHIFT:
            r = self.range >> tot
            top = (lt + sy) >> tot
        else:
            r = self.range // tot
            top = lt + sy >= tot
        self.low += r * lt
        self.range = self.range - r * lt if top else r * sy


def _pending_run(nmax):
    """steps that put the carry boundary (2^31 of the interval's scale) strictly inside the interval and keep it there, one byte
    shift and one more pending 0xFF per step.  Returns (steps, state in front of step i for every i)"""
    sim, steps, states = _Sim(), [], []

    def inside(tots):        # the part of the interval (sy = 1 of tot) that holds the boundary, which must not sit on its edge
        sim.normalize()
        d = (1 << 31) - sim.low
        assert 0 < d < sim.range
        for tot in tots:
            r = sim.range // tot
            lt = min(d // r, tot - 1)          # (the last part also takes the division's remainder)
            if d - r * lt > 0 and (1 << 15) < r <= (1 << 23) - 256:
                return freq(1, lt, tot)
        raise AssertionError("no step keeps the boundary inside")

    # [0, 2^31) -> its middle third -> the 255th of it that holds 0x40000000: behind the byte shift the boundary is inside
    for w in (freq(1, 1, 3), None):
        if w is None:
            r = sim.range // 255
            d = 0x40000000 - sim.low
            assert d % r
            w = freq(1, d // r, 255)
        states.append(sim.copy())
        steps.append(w)
        sim.step(w)
    sim.normalize()
    assert sim.help == 0 and sim.low + sim.range > (1 << 31) > sim.low
    while len(steps) < nmax + 2:
        sim.normalize()
        w = inside((257, 259, 263, 300) if sim.range > (1 << 30) else (255, 253, 251, 200))      # one byte shift per step
        states.append(sim.copy())
        steps.append(w)
        sim.step(w)
        assert (1 << 15) < sim.range <= (1 << 23)
    states.append(sim.copy())
    return steps, states


C1_RUNS = (1, 2, 255, 256, 32766, 32767, 32768, 32769, 32770, 65535, 65536, 65537, 70000)


def _c1():
    out = []
    steps, states = _pending_run(max(C1_RUNS) + 8)
    filler = [shift(1, 0, 1), shift(1, 0, 8), freq(1, 0, 3), shift(3, 0, 8)]       # (lt = 0: low stays, no carry of their own)
    for run in C1_RUNS:
        # the first two steps open the run; step i + 2 finds i bytes pending.  `run` bytes are pending in front of step run + 2
        n = run + 2
        sim = states[n].copy()
        sim.normalize()
        assert sim.help == run
        d, R = (1 << 31) - sim.low, sim.range
        # (a) a step whose interval lies above the boundary: the carry runs through all pending bytes
        tot = next(t for t in (255, 64, 16, 4, 3) if d // (R // t) + 1 < t - 1)
        out.append({"family": "C1", "name": "C1-run%d-carry" % run, "first_byte": 0x80,
                    "steps": steps[:n] + [freq(1, d // (R // tot) + 1, tot)] + filler, "expect": {"carries": 1, "finish_carry": 0, "min_help": run}})
        # (b) a step whose interval lies below it, by more than a byte's worth: the pending bytes leave as 0xFF
        tot = next(t for t in (255, 1000, 60000) if d > R // t + (1 << 23))
        out.append({"family": "C1", "name": "C1-run%d-nocarry" % run, "first_byte": 0x80, "steps": steps[:n] + [freq(1, 0, tot)] + filler,
                    "expect": {"carries": 0, "finish_carry": 0, "min_help": run}})
        # (c) finish with the boundary still inside: search a last step behind which finish rounds low up into the carry
        found = None
        for back in range(0, 6):
            base = states[n + back].copy()
            base.normalize()
            for sh in range(1, 9):
                dd, rr = (1 << 31) - base.low, base.range >> sh
                if rr == 0 or dd % rr == 0 or dd // rr + 1 > (1 << sh) - 1:
                    continue
                w = shift(1, dd // rr, sh)
                t = base.copy()
                t.step(w)
                t.normalize()
                count = 1 + (n + back + 1) + 64          # finish compares the low bits with about half the byte count
                if (t.low >> 23) == 0xFF and (t.low & 0x7FFFFF) >= count and not (t.low & (1 << 31)):
                    found = steps[: n + back] + [w]
                    break
            if found:
                break
        assert found is not None
        out.append({"family": "C1", "name": "C1-run%d-finish" % run, "first_byte": 0x80, "steps": found,
                    "expect": {"carries": 1, "finish_carry": 1, "min_help": run}})
    # the literal run: shift(1, 255, 8) behind shift(1, 1, 1) keeps low at 0x7FC00000 with the interval's top ON the boundary
    for run in (1, 2, 255, 256, 32767, 32768, 65536, 70000):
        out.append({"family": "C1", "name": "C1-literal-run%d" % run, "first_byte": 0x81,
                    "steps": [shift(1, 1, 1)] + [shift(1, 255, 8)] * run + [shift(1, 0, 8), shift(1, 3, 8)],
                    "expect": {"carries": 0, "finish_carry": 0, "min_help": run}})
    return out


def _c2():
    out = []
    rng = np.random.RandomState(99)
    # shift(1, b, 7) leaves range = 2^24; a freq step of sy = 1 under a total near 2^17 then leaves 128: three byte shifts
    three, two = [], []
    for tot in (0x1FFFF, 0xFFFF, 0xFF00):
        for k in range(40):
            lt = int(rng.randint(0, min(tot - 1, 0xFFFF)))
            three += [shift(1, int(rng.randint(0, 127)), 7), freq(1, lt, tot)]
            two.append(freq(1, int(rng.randint(0, 0xFFFF)), 0xFFFF))      # range 2^31 -> 2^15 -> two shifts -> 2^31
    out.append({"family": "C2", "name": "C2-three-shifts", "first_byte": 0x80, "steps": three, "expect": {"max_shifts": 3}})
    out.append({"family": "C2", "name": "C2-two-shifts", "first_byte": 0xFF, "steps": two, "expect": {"max_shifts": 2}})
    small = []
    for k in range(200):
        small += [freq(1, 0, 1), freq(1, int(rng.randint(0, 2)), 2), freq(2, 0, 2), freq(1, int(rng.randint(0, 3)), 3)]
    out.append({"family": "C2", "name": "C2-totals-1-2", "first_byte": 0x80, "steps": small, "expect": {}})
    top = []
    for k in range(300):
        tot = int(rng.randint(2, 1 << 17))
        sy = int(rng.randint(1, min(tot, 0xFFFF) + 1))
        if tot - sy > 0xFFFF:
            sy = tot - 0xFFFF
        top.append(freq(sy, tot - sy, tot))                 # lt + sy == tot: range - tmp
        top.append(shift(1, 255, 8) if k % 3 == 0 else shift(1, 1, 1))
    out.append({"family": "C2", "name": "C2-top-branch", "first_byte": 0x80, "steps": top, "expect": {}})
    out.append({"family": "C2", "name": "C2-mixed", "first_byte": 0x93, "steps": two[:60] + three[:60] + small[:100] + top[:100] + two[:60],
                "expect": {"max_shifts": 3}})
    return out


C3_LEN = (0, 1, 32766, 32767, 32768, 32769, 200000)


def random_steps(n, seed):
    rng = np.random.RandomState(seed)

    def below(bound):                          # uniform in [0, bound) per element
        return rng.randint(0, 1 << 40, n) % bound
    tot = rng.randint(1, 1 << 17, n)
    sy = 1 + below(np.minimum(tot, 0xFFFF))
    lt = below(np.minimum(tot - sy, 0xFFFF) + 1)
    w = (sy | (lt << 16) | (tot << 32)).astype(np.uint64)
    sh = np.where(rng.randint(0, 2, n) == 0, 1, 8)
    ssy = 1 + below(1 << sh)
    slt = below((1 << sh) - ssy + 1)
    ws = (ssy | (slt << 16) | (sh << 32)).astype(np.uint64) | np.uint64(SHIFT)
    return np.where(rng.randint(0, 4, n) == 0, ws, w)


def _c3():
    return [{"family": "C3", "name": "C3-n%d-seed%d" % (n, s), "first_byte": (0x80 + 37 * s) & 0xFF, "steps": random_steps(n, 100 * s + 7),
             "expect": {}} for n in C3_LEN for s in ((1, 2) if n < 100000 else (1,))]


C4_GOLDEN = (("sample1", 9), ("long_runs_mixed", 1), ("sample3", 1))       # cases of golden_small.json (sample3 at level 1: two blocks)


def golden_input(name):
    case = next(c for c in support.load_golden("golden_small.json")["cases"] if c["name"] == name and c["algo"] == "BWTC")
    return recipes.build(case["recipe"])


def _c4():
    out = []
    for name, level in C4_GOLDEN:
        rc, steps, _, fb, _ = oracle().bwtc_stream_steps(golden_input(name), level)
        assert rc == 0
        out.append({"family": "C4", "name": "C4-%s-level%d" % (name, level), "first_byte": fb, "steps": steps, "expect": {}})
    return out


_CODER = None


def coder_cases():
    global _CODER
    if _CODER is None:
        _CODER = _c1() + _c2() + _c3() + _c4()
        for c in _CODER:
            c["steps"] = np.asarray(c["steps"], dtype=np.uint64)
    return _CODER
