"""The crafted-header cases shared by test_bzcraft_host.py (no GPU: model == oracle, and every case is what it claims) and
test_gpu_crafted_headers.py (the HIP decoder == the oracle).  Families: U used map, S selectors, L code lengths, T canonical
tables, C the group chain under different tables, M inverse MTF on large alphabets, B the level pairs of the batch test.

A case: name, make() -> a block or a list of blocks (bzcraft.block), expect ('ok' or the model's name of the reference check that
rejects it with its line, e.g. 'selector:1490'), claim(blocks) -> asserts from the writer's offsets that the case reaches the
seam it is named after; level: the stream header's digit; tail: bytes behind the stream.
"""
import numpy as np

import bzcraft
from bzcraft import RUNA, RUNB, STRETCH, block

CH_WINDOW_BITS = 65536        # csrc/decode_dev.h: 32 * CH_WORDS, the bits of the stream bz_chain keeps in LDS between refills


class Case:
    def __init__(self, name, make, expect="ok", claim=None, level=9, tail=b""):
        self.name, self.family, self.expect, self.claim, self.level, self.tail = name, name[0], expect, claim, level, tail
        self._make, self._built = make, None

    def blocks(self):
        if self._built is None:
            made = self._make()
            self._built = made if isinstance(made, list) else [made]
        return self._built

    def stream(self):
        return bzcraft.stream(self.blocks(), self.level, self.tail)


# ---------------------------------------------------------------- pieces
def complete(n):
    """n code lengths with Kraft sum 1 (n >= 2)"""
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def rolled(lengths, by):
    by %= len(lengths)
    return lengths[by:] + lengths[:by]


def tab(lengths, **kw):
    return dict(lengths=list(lengths), **kw)


def run_digits(n):
    """the RUNA / RUNB digits of a run of n bytes (bijective base 2, lowest digit first)"""
    out = []
    while n:
        if n & 1:
            out.append(RUNA)
            n -= 1
        else:
            out.append(RUNB)
            n -= 2
        n >>= 1
    return out


def mtf_values(tables_wanted, count):
    """the unary values that select the wanted tables (each < count)"""
    lst = list(range(count))
    out = []
    for t in tables_wanted:
        j = lst.index(t)
        out.append(j)
        lst.insert(0, lst.pop(j))
    return out


def ranks(rng, n_used, count, run_every=0):
    """`count` rank symbols 2 .. n_used (n_used >= 2), a short zero-rank run in front of every run_every-th"""
    out = []
    for i in range(count):
        if run_every and i % run_every == run_every - 1:
            out += run_digits(int(rng.randint(1, 40)))
        out.append(int(rng.randint(2, n_used + 1)))
    return out


def n_groups(symbols):
    return (len(symbols) + 1 + 49) // 50            # (with the end-of-block symbol)


def plain(used, symbols, n_tables=2, selectors=None, **kw):
    """a block under complete tables (table t: the lengths rolled by t), selectors 0 unless given"""
    n = len(set(used)) + 2
    sel = [0] * n_groups(symbols) if selectors is None else selectors
    return block(used=used, tables=[tab(rolled(complete(n), t)) for t in range(n_tables)], selectors=sel, symbols=symbols, **kw)


def sel_text(b):
    return b.text(*b.sel)


def tab_text(b, t):
    return b.text(b.tab[t][1], b.tab[t][2])        # from the stretch origin (behind the 5-bit start) to the table's end


def group_bits(b):
    return [y - x for x, y in zip(b.groups, b.groups[1:] + [b.end])]


def has(cond, what=""):
    assert cond, what


CASES = []


def case(name, make, expect="ok", claim=None, **kw):
    CASES.append(Case(name, make, expect, claim, **kw))


# ---------------------------------------------------------------- U: the used map
def _u_none(symbols, crc_of=None, **kw):
    return lambda: block(used=(), tables=[tab([1, 1]), tab([1, 1])], selectors=[0, 1], symbols=symbols, eob=False,
                         crc=None if crc_of is None else bzcraft._crc(crc_of), **kw)


_no_row = lambda bs: has(bs[0].text(105, 121) == "0" * 16 and bs[0].sel[0] == 105 + 16 + 18, "no coarse bit, no fine word")          # noqa: E731
case("U-none", _u_none([RUNA, RUNB] * 10), "selectors-run-out:1601", _no_row)
# (a decoder that took RUNB for the end of block -- it is symbol sym_total + 1 here -- would emit one byte 0: give it that CRC)
case("U-none-crc-of-a-zero-byte", _u_none([RUNA, RUNB], crc_of=b"\0"), "selectors-run-out:1601", _no_row)
case("U-randomised-bit", lambda: plain((97, 98, 99), [2, 3, 4, RUNA] * 10, randomised=1), "randomised:1446", lambda bs: has(bs[0].text(80, 81) == "1"))
for _v in (0, 255, 200):
    case("U-one-%d" % _v, lambda v=_v: block(used=(v,), tables=[tab([2, 1, 2]), tab([1, 2, 2])], selectors=[1, 0],
                                             symbols=[RUNA, RUNB] * 32 + [RUNB, RUNA, RUNB], orig=5),      # 64 digits forgotten, then 2 + 2 + 8 bytes
         claim=lambda bs: has(bs[0].sel[0] == 105 + 16 + 16 + 18 and len(bs[0].groups) == 2))
case("U-256", lambda: plain(range(256), ranks(np.random.RandomState(1), 256, 600, 7) + [257 - 1, 2, 256]),
     claim=lambda bs: has(bs[0].sel[0] == 105 + 16 + 256 + 18))
case("U-each-row", lambda: plain([16 * r + (7 * r) % 16 for r in range(16)], ranks(np.random.RandomState(2), 16, 300, 5)),
     claim=lambda bs: has(bs[0].sel[0] == 105 + 16 + 256 + 18))
case("U-empty-fine-word", lambda: plain((97, 98, 99), ranks(np.random.RandomState(3), 3, 120, 4), empty_rows=(2, 15)),
     claim=lambda bs: has(bs[0].text(121, 137) == "0" * 16 and bs[0].sel[0] == 105 + 16 + 48 + 18, "row 2 is the first fine word"))
case("U-last-row", lambda: plain((240, 250, 255), ranks(np.random.RandomState(4), 3, 120, 4)),
     claim=lambda bs: has(bs[0].text(105, 121) == "0" * 15 + "1"))


# ---------------------------------------------------------------- S: selectors
def _s_block(count, values, n_sel=None, seed=0, real=None, group_count=None):
    """`count` complete tables over 5 symbols; `real` groups of symbols (default: one per value), the other selectors are spare"""
    rng = np.random.RandomState(100 + seed)
    real = len(values) if real is None else real
    symbols = ranks(rng, 3, 50 * real - 8, 6)
    symbols = symbols[: 50 * real - 1]
    return block(used=(65, 66, 67), tables=[tab(rolled(complete(5), t)) for t in range(count)], selectors=values, symbols=symbols,
                 n_sel=n_sel, group_count=group_count)


for _g in range(2, 7):
    _vals = [int(x) for x in np.random.RandomState(_g).randint(0, _g, 40)] + list(range(_g)) + [_g - 1] * 3
    case("S-count%d-every-value" % _g, lambda g=_g, v=_vals: _s_block(g, v, seed=g),
         claim=lambda bs, g=_g, v=_vals: has(set(v) == set(range(g)) and set(bs[0].sel_tables) == set(range(g))
                                            and sel_text(bs[0]) == "".join("1" * x + "0" for x in v)))
for _name, _g, _vals in (("first", 3, [3, 1, 2, 0, 1]), ("middle", 3, [1, 2, 3, 2, 0, 1]), ("twice", 4, [2, 4, 4, 1, 3, 4, 0]),
                         ("six-tables", 6, [5, 6, 3, 6, 6, 5, 6, 1]), ("two-tables", 2, [1, 2, 2, 1, 2, 0])):
    case("S-value-equals-count-" + _name, lambda g=_g, v=_vals: _s_block(g, v, seed=7),
         claim=lambda bs, g=_g, v=_vals: has(bs[0].sel_tables[v.index(g)] == 0 and "1" * g + "0" in sel_text(bs[0]),
                                            "the first value equal to the count selects table 0 (the zero slot behind the tables)"))
for _g in (2, 6):
    case("S-value-above-count-%d" % _g, lambda g=_g: _s_block(g, [0, 1, g + 1, 0], seed=8), "selector:1490",
         claim=lambda bs, g=_g: has("1" * (g + 1) + "0" in sel_text(bs[0])))
case("S-count-1", lambda: _s_block(2, [0, 0], group_count=1), "group-count:1471")
case("S-count-7", lambda: _s_block(6, [0, 0], group_count=7), "group-count:1471")
case("S-nsel-0", lambda: _s_block(2, [0, 0], n_sel=0), "n-sel:1478")

S_NSEL = (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32767)
for _n in S_NSEL:
    # one real group, the other selectors are spare: behind the end of block the chain walks the zero bits past the stream's end
    _vals = [int(x) for x in np.random.RandomState(300 + _n).randint(0, 6, _n)]
    case("S-nsel-%d" % _n, lambda v=_vals: _s_block(6, v, real=1),
         claim=lambda bs, n=_n: has(sel_text(bs[0]).count("0") == n and int(bs[0].text(bs[0].sel[0] - 15, bs[0].sel[0]), 2) == n
                                   and len(bs[0].groups) == 1))
S_SHIFT_LIST = [5, 0, 0, 3, 5, 5, 1, 0, 4, 2, 5, 0, 0, 0, 5, 3, 1, 5, 4, 0, 2, 5, 5, 5, 0, 1, 3, 0, 4, 5, 2, 0] * 3
for _k in range(32):
    # the list behind k spare selectors of value 0: every zero and every run of ones meets every border of the lanes' 32-bit words
    case("S-shift-%d" % _k, lambda k=_k: _s_block(6, [0] * k + S_SHIFT_LIST, real=2, seed=_k),
         claim=lambda bs, k=_k: has(sel_text(bs[0])[k:] == "".join("1" * x + "0" for x in S_SHIFT_LIST) and sel_text(bs[0])[:k] == "0" * k))
for _k in range(32):
    # the same block behind a block that is k bits longer each time: the header sections start at every bit of a 32-bit word of
    # the input (the lanes' loads are funnel shifts of two aligned words)
    case("S-second-block-at-bit-%d" % _k,
         lambda k=_k: [_s_block(3, [2, 0, 1] + [0] * k, real=2, seed=50), _s_block(6, S_SHIFT_LIST, real=2, seed=51),
                       plain(range(256), ranks(np.random.RandomState(52), 256, 60, 5))],
         claim=lambda bs, k=_k: has(bs[0].bits.size == bs[0].end and bs[0].sel[1] - bs[0].sel[0] == 6 + k))
for _d in range(1, 6):
    def _cross(d=_d):
        vals, bits = [], 0
        rng = np.random.RandomState(400 + d)
        while bits < STRETCH + d - 6 - 8:
            v = int(rng.randint(0, 5))
            vals.append(v)
            bits += v + 1
        while bits < STRETCH + d - 6:                 # single zeros up to the run's first bit
            vals.append(0)
            bits += 1
        return _s_block(6, vals + [5] + [int(x) for x in rng.randint(0, 6, 30)], real=3, seed=d)
    case("S-run-crosses-stretch-%d" % _d, _cross,
         claim=lambda bs, d=_d: has(len(sel_text(bs[0])) > STRETCH and sel_text(bs[0])[STRETCH + d - 6: STRETCH + d] == "111110",
                                   "a value 5 whose zero is bit %d of the second stretch" % (d - 1)))


# ---------------------------------------------------------------- L: code lengths
def _l_block(tables, used=(65, 66, 67), selectors=None, symbols=None, seed=0):
    rng = np.random.RandomState(500 + seed)
    n_used = len(set(used))
    symbols = ranks(rng, n_used, 170, 5) if symbols is None else symbols
    return block(used=used, tables=tables, selectors=([0, 1] * n_groups(symbols))[: n_groups(symbols)] if selectors is None else selectors, symbols=symbols)


case("L-start-1", lambda: _l_block([tab([1, 2, 3, 4, 4]), tab([3, 3, 2, 2, 2], start=1)]),
     claim=lambda bs: has(bs[0].text(bs[0].tab[0][0], bs[0].tab[0][1]) == "00001" and bs[0].text(bs[0].tab[1][0], bs[0].tab[1][1]) == "00001"))
case("L-start-20", lambda: _l_block([tab([20, 20, 1, 20, 20]), tab([3, 3, 2, 2, 2], start=20)]),
     claim=lambda bs: has(bs[0].text(bs[0].tab[0][0], bs[0].tab[0][1]) == "10100" and bs[0].text(bs[0].tab[1][0], bs[0].tab[1][1]) == "10100"))
GARBAGE = "1011001110001111" * 8
case("L-start-0", lambda: _l_block([tab(complete(5)), tab(complete(5), raw="00000" + "0" * 5 + GARBAGE)]), "length:1509")
case("L-start-21", lambda: _l_block([tab(complete(5), raw="10101" + "0" * 5 + GARBAGE), tab(complete(5))]), "length:1509")
case("L-walk-to-0", lambda: _l_block([tab(complete(5)), tab(complete(5), raw="00010" + "0" + "110" + "11" + GARBAGE)]), "length:1509",
     claim=lambda bs: has(tab_text(bs[0], 1).startswith("011011")))
case("L-walk-to-21", lambda: _l_block([tab(complete(5)), tab(complete(5), raw="10011" + "0" + "100" + "10" + GARBAGE)]), "length:1509",
     claim=lambda bs: has(tab_text(bs[0], 1).startswith("010010")))
for _k in (0, 5, 13, 26, 31):
    # 20 -> 0 (40 ones) behind k symbols, then ones: whole lane words of ones next to each other.  (A string the reference reads to
    # its end has no more than 38 ones in a row -- 20 down to 1 -- so two such words next to each other exist only here.)
    case("L-walk-to-0-ones-%d" % _k,
         lambda k=_k: _l_block([tab(complete(42)), tab(complete(42), raw="10100" + "0" * k + "1" * 40 + "1" * 150 + "0" * 40)], used=range(40)),
         "length:1509",
         claim=lambda bs: has(sum(1 for x, y in zip(bs[0].lane_words(bs[0].tab[1][1], bs[0].tab[1][2]), bs[0].lane_words(bs[0].tab[1][1], bs[0].tab[1][2])[1:])
                                  if x == y == "1" * 32) >= 1, "two all-ones lane words next to each other"))
for _z in (1, 3, 40):
    case("L-zig-%d" % _z, lambda z=_z: _l_block([tab(complete(5), zig=z), tab(rolled(complete(5), 2), zig=z)]),
         claim=lambda bs, z=_z: has(tab_text(bs[0], 0).count("1011") >= 5 * z and len(tab_text(bs[0], 1)) >= 5 * (4 * z + 1)))
L_ALT = lambda k: [20] * (1 + k) + [1 if i % 2 == 0 else 20 for i in range(257 - k)]          # noqa: E731
for _k in range(32):
    case("L-alternating-shift-%d" % _k,
         lambda k=_k: _l_block([tab(complete(258)), tab(rolled(complete(258), 9)), tab(L_ALT(k))], used=range(256),
                               symbols=ranks(np.random.RandomState(600 + k), 256, 120, 6)),
         claim=lambda bs, k=_k: has("1" * 38 + "0" in tab_text(bs[0], 2) and "1" * 39 not in tab_text(bs[0], 2) and len(tab_text(bs[0], 2)) > 2 * STRETCH
                                   and tab_text(bs[0], 2).startswith("0" * (1 + k) + "1" * 38)))
case("L-longer-than-2048", lambda: _l_block([tab(complete(258), zig=2), tab(rolled(complete(258), 100), zig=2)], used=range(256),
                                            symbols=ranks(np.random.RandomState(7), 256, 170, 6)),
     claim=lambda bs: has(STRETCH < len(tab_text(bs[0], 0)) < 2 * STRETCH and len(tab_text(bs[0], 1)) > STRETCH))
case("L-longer-than-4096", lambda: _l_block([tab(complete(258), zig=4), tab(rolled(complete(258), 100), zig=5)], used=range(256),
                                            symbols=ranks(np.random.RandomState(8), 256, 170, 6)),
     claim=lambda bs: has(len(tab_text(bs[0], 0)) > 2 * STRETCH and len(tab_text(bs[0], 1)) > 2 * STRETCH))
# 258 symbols, one step up and 447 zig pairs: 258 + 2 + 4 * 447 = 2048 bits; 257 symbols and 448 pairs: 257 + 4 * 448 = 2049
case("L-ends-on-last-bit-of-stretch",
     lambda: _l_block([tab([9] + [10] * 257, zig=[2] * 189 + [1] * 69), tab(complete(258))], used=range(256), symbols=ranks(np.random.RandomState(9), 256, 170, 6)),
     claim=lambda bs: has(len(tab_text(bs[0], 0)) == STRETCH))
case("L-ends-on-first-bit-of-next-stretch",
     lambda: _l_block([tab([10] * 257, zig=[2] * 191 + [1] * 66), tab(complete(257))], used=range(255), symbols=ranks(np.random.RandomState(10), 255, 170, 6)),
     claim=lambda bs: has(len(tab_text(bs[0], 0)) == STRETCH + 1))


# ---------------------------------------------------------------- T: canonical tables
def _t_block(lengths, used, symbols, other=None, **kw):
    sel = [0, 1] * ((n_groups(symbols) + 1) // 2) if other is not None else [0] * n_groups(symbols)
    return block(used=used, tables=[tab(lengths), tab(lengths if other is None else other)], selectors=sel, symbols=symbols, **kw)


case("T-all-2-bits-3-symbols", lambda: _t_block([2, 2, 2], (9,), [RUNA, RUNB] * 4),
     claim=lambda bs: has(group_bits(bs[0]) == [18]))
case("T-all-20-bits-3-symbols", lambda: _t_block([20, 20, 20], (9,), [RUNA] * 64 + [RUNB, RUNA, RUNB]),
     claim=lambda bs: has(group_bits(bs[0]) == [1000, 360]))
case("T-all-9-bits-258-symbols", lambda: _t_block([9] * 258, range(256), ranks(np.random.RandomState(11), 256, 300, 9)),
     claim=lambda bs: has(all(g % 9 == 0 for g in group_bits(bs[0]))))
case("T-lengths-10-and-11", lambda: _t_block([10] * 100 + [11] * 158, range(256), ranks(np.random.RandomState(12), 256, 300, 9), other=[11] * 158 + [10] * 100),
     claim=lambda bs: has(500 < min(group_bits(bs[0])[:-1]) and max(group_bits(bs[0])) < 550))
case("T-lengths-12-and-13", lambda: _t_block([12] * 100 + [13] * 158, range(256), ranks(np.random.RandomState(13), 256, 300, 9), other=[13] * 158 + [12] * 100),
     claim=lambda bs: has(600 < min(group_bits(bs[0])[:-1]) and max(group_bits(bs[0])) <= 650))
case("T-only-long-code-is-20-bits", lambda: _t_block([1, 2, 3, 4, 20], (65, 66, 67), [2, 3, RUNA, 3, RUNB, 2, 3] * 30, other=[20, 4, 3, 2, 1]),
     claim=lambda bs: has(max(group_bits(bs[0])) < 400))
HOLE = [2, 2, 3, 3, 3]                              # codes 00 01 100 101 110: nothing decodes 111
case("T-hole-never-met", lambda: _t_block(HOLE, (65, 66, 67), ranks(np.random.RandomState(14), 3, 200, 5)),
     claim=lambda bs: has("111" not in {bzcraft.Table(HOLE).code(s) for s in range(5)}))
case("T-hole-in-first-group", lambda: _t_block(HOLE, (65, 66, 67), [2, 3, 2, "111"] + [3] * 100), "no-code:1608",
     claim=lambda bs: has(bs[0].text(bs[0].groups[0], bs[0].groups[0] + 11) == "100" + "101" + "100" + "11"[:2]))
case("T-hole-in-later-group", lambda: _t_block(HOLE, (65, 66, 67), [2, 3] * 60 + ["111"] + [3] * 100), "no-code:1608",
     claim=lambda bs: has(len(bs[0].groups) > 3 and bs[0].text(bs[0].groups[2] + 60, bs[0].groups[2] + 63) == "111"))
# spare selectors: behind the end of block the chain meets the stream's end magic and then ones, which HOLE cannot decode
case("T-hole-behind-end-of-block", lambda: block(used=(65, 66, 67), tables=[tab(HOLE), tab(HOLE)], selectors=[0, 1, 0, 0, 1, 1, 0, 0],
                                                symbols=ranks(np.random.RandomState(15), 3, 120, 5)),
     claim=lambda bs: has(len(bs[0].groups) < len(bs[0].sel_tables) == 8), tail=b"\xff" * 160)
case("T-oversubscribed-2-2-1-2-1", lambda: _t_block([2, 2, 1, 2, 1], (65, 66, 67), [2] * 120),
     claim=lambda bs: has(group_bits(bs[0]) == [50, 50, 21]))
case("T-oversubscribed-three-levels", lambda: _t_block([3, 2, 2, 2, 1], (65, 66, 67), [2, RUNB, 2, 2, RUNB, RUNB, 2] * 20),
     claim=lambda bs: has(group_bits(bs[0])[0] == 100))


# ---------------------------------------------------------------- C: the chain under different tables
# six symbols (four used bytes); shortest / longest code (1, 1), (1, 20), (11, 13), (20, 20), (2, 9), (2, 3).  Under table 0 only
# RUNA and RUNB have codes: a group of it is 50 digits of a zero-rank run, which the reference forgets every 32 digits (the int32
# weight): the group behind m such groups opens with -50 m mod 32 digits more, and nothing is left of the run.
C_TABLES = ([1] * 6, [20, 20, 1, 20, 20, 20], [11, 12, 11, 13, 12, 13], [20] * 6, [2, 9, 2, 3, 9, 9], [2, 2, 3, 3, 3, 3])
C_USED = (65, 66, 67, 68)


def _c_symbols(rng, seq):
    """50 symbols for every table of `seq` (the last group one short: the end-of-block symbol); seq must not end in table 0"""
    out, pending = [], 0
    for t in seq:
        if t == 0:
            out += [int(x) for x in rng.randint(0, 2, 50)]
            pending += 50
            continue
        head = [RUNA] * (-pending % 32)
        pending = 0
        body = [int(x) for x in rng.randint(2, 5, 50 - len(head))]
        if t == 1:                                  # groups of 50 .. 1000 bits
            p = rng.random_sample()
            body = [2 if x < p else 3 for x in rng.random_sample(50 - len(head))]
        for at in rng.randint(1, len(body) - 1, 2):
            body[at] = int(rng.randint(0, 2))       # (a digit or two of a run inside)
        body[0] = body[-1] = 2 if t == 1 else int(rng.randint(2, 5))
        out += head + body
    return out[:-1]


def _c_block(seq, seed, count=6):
    rng = np.random.RandomState(800 + seed)
    return block(used=C_USED, tables=[tab(C_TABLES[t]) for t in range(count)], selectors=mtf_values(seq, count), symbols=_c_symbols(rng, seq))


def _neighbours(b, n):
    s = b.sel_tables[: len(b.groups)]
    return {tuple(s[i: i + n]) for i in range(len(s) - n + 1)}


for _count in (3, 4, 5, 6):
    _seq = [b for a in range(_count) for b in (a, a, (a + 1) % _count)] + [a2 for a in range(_count) for b in range(_count) for a2 in (a, b)] + [1]
    case("C-every-pair-of-%d-tables" % _count, lambda s=_seq, c=_count: _c_block(s, c, c),
         claim=lambda bs, c=_count: has(_neighbours(bs[0], 2) >= {(a, b) for a in range(c) for b in range(c)}))
for _seed in range(12):
    _seq = [int(x) for x in np.random.RandomState(900 + _seed).randint(0, 6, 300)] + [5]
    case("C-mix-seed%d" % _seed, lambda s=_seq, seed=_seed: _c_block(s, 20 + seed),
         claim=lambda bs: has(len(bs[0].groups) == 301 and len(_neighbours(bs[0], 3)) > 120 and min(group_bits(bs[0])[:-1]) == 50 and max(group_bits(bs[0])) == 1000))


def group_of_bits(bits, n=50):
    """n rank symbols whose codes (20, 10 and 1 bits under lengths [20, 20, 1, 10, 20, 20]) take exactly `bits` bits"""
    for a in range(n, -1, -1):                      # 19 a + 9 c = bits - n
        rest = bits - n - 19 * a
        if rest >= 0 and rest % 9 == 0 and a + rest // 9 <= n:
            c = rest // 9
            return [4] * a + [3] * c + [2] * (n - a - c)
    raise ValueError(bits)


C_LENGTHS = [50, 1000, 50, 449, 448, 50, 449, 1000, 1000, 50, 50, 50, 1000, 449, 449, 59, 1000, 1000, 1000, 1000, 50, 1000, 448, 448, 1000, 50]
case("C-group-lengths-next-to-each-other",
     lambda: block(used=C_USED, tables=[tab([20, 20, 1, 10, 20, 20]), tab([20] * 6)], selectors=mtf_values([0] * len(C_LENGTHS) + [1, 1, 1, 1, 0], 2),
                   symbols=[x for g in C_LENGTHS for x in group_of_bits(g)] + [2, 3, 4, 2, 5 - 1] * 40 + [2] * 49),
     claim=lambda bs: has(group_bits(bs[0])[: len(C_LENGTHS)] == C_LENGTHS and group_bits(bs[0])[len(C_LENGTHS):] == [1000] * 4 + [50 + 19]))
case("C-groups-of-447-448-449-bits",
     lambda: block(used=C_USED, tables=[tab([20, 20, 1, 10, 20, 20])] * 2, selectors=[0] * 13,
                   symbols=[x for g in [59, 447, 447, 447, 447, 59, 448, 448, 448, 448, 449, 449] for x in group_of_bits(g)] + group_of_bits(448, 49)),
     claim=lambda bs: has(group_bits(bs[0])[:12] == [59, 447, 447, 447, 447, 59, 448, 448, 448, 448, 449, 449]))
for _n in (5, 6, 7, 8):
    # every group 150 bits under 3-bit codes: the chain takes four groups a step, the last step holds n - 4
    case("C-last-step-holds-%d" % (_n - 4), lambda n=_n: block(used=(1, 2, 3, 4, 5, 6), tables=[tab([3] * 8)] * 2, selectors=[0, 1] * (n // 2) + [0] * (n % 2),
                                                               symbols=ranks(np.random.RandomState(n), 6, 50 * n - 1)),
         claim=lambda bs, n=_n: has(group_bits(bs[0]) == [150] * n))
C_REFILL_FLIPS = {495, 496, 497, 511, 512, 513, 1007, 1008, 1009, 1023, 1024, 1025}
case("C-selector-refill-at-512", lambda: block(used=C_USED, tables=[tab(C_TABLES[5]), tab(C_TABLES[4])],
                                               selectors=mtf_values([1 if (i in C_REFILL_FLIPS) != (i % 2 == 1 and 490 < i < 520) else 0 for i in range(1100)], 2),
                                               symbols=ranks(np.random.RandomState(31), 4, 50 * 1100 - 1, 11)[: 50 * 1100 - 1]),
     claim=lambda bs: has(len(bs[0].groups) == 1100 and bs[0].sel_tables[494:499] != [bs[0].sel_tables[494]] * 5
                          and len(set(bs[0].sel_tables[510:515])) == 2 and len(set(bs[0].sel_tables[1006:1011])) == 2))


def _window_block():
    seq = [1, 5, 3, 1] + [3] * 70 + [1, 3, 1, 3, 3, 1, 1, 3] * 2 + [5] * 4
    return _c_block(seq, 40)


case("C-window-refill-among-1000-bit-groups", _window_block,
     claim=lambda bs: has(bs[0].end - bs[0].groups[0] > CH_WINDOW_BITS
                          and all(g == 1000 for g, at in zip(group_bits(bs[0]), bs[0].groups) if CH_WINDOW_BITS - 6000 < at - bs[0].groups[0] < CH_WINDOW_BITS + 3000)))


# ---------------------------------------------------------------- M: inverse MTF on large alphabets
M_MAPS = {"256": list(range(256)), "200": [b for b in range(256) if (b * 7) % 32 < 25]}
assert len(M_MAPS["200"]) == 200


def _m_block(used, symbols):
    n = len(used) + 2
    sel = [0, 1, 1, 0, 1] * (n_groups(symbols) // 5 + 1)
    return block(used=used, tables=[tab(complete(n)), tab([9] * n)], selectors=sel[: n_groups(symbols)], symbols=symbols)


def _m_case(name, key, symbols, n_ops=None):
    used = M_MAPS[key]
    want = sum(1 for s in symbols if s >= 2) if n_ops is None else n_ops
    case("M-%s-%s" % (key, name), lambda: _m_block(used, symbols),
         claim=lambda bs: has(sum(1 for s in symbols if s >= 2) == want and len(bs[0].groups) == n_groups(symbols)
                              and bs[0].sel[0] == 105 + 16 + 256 + 18))


for _key in ("256", "200"):
    _top = len(M_MAPS[_key])                        # the rank symbol of the list's last slot
    _m_case("last-rank-throughout", _key, [_top] * 700)
    _m_case("ranks-3-4-5", _key, [4, 5, 6, 4, 6, 5, 5, 4, 6, 6, 4] * 60)
    if _key == "256":
        _m_case("ranks-251-252-253", _key, [252, 253, 254, 252, 254, 253, 253, 252, 254, 254, 252] * 60)
    else:
        _m_case("ranks-195-196-197", _key, [196, 197, 198, 196, 198, 197, 197, 196, 198, 198, 196] * 60)
    for _n in (255, 256, 257, 16383, 16384, 16385, 32769):
        _rng = np.random.RandomState(1000 + _n)
        _m_case("ops-%d" % _n, _key, [int(x) for x in _rng.randint(2, _top + 1, _n)], n_ops=_n)
    _m_case("run-in-front-of-first-op", _key, run_digits(37) + [int(x) for x in np.random.RandomState(5).randint(2, _top + 1, 300)])
    _m_case("runs-of-16-and-17-behind-ops", _key, [x for i in range(200) for x in [2 + (i * 37) % (_top - 1)] + run_digits(16 + i % 2)])
    _m_case("run-of-5000-behind-last-op-of-tile", _key,
            [int(x) for x in np.random.RandomState(6).randint(2, _top + 1, 256)] + run_digits(5000) + [int(x) for x in np.random.RandomState(7).randint(2, _top + 1, 300)],
            n_ops=556)


# ---------------------------------------------------------------- B: the level pairs of the batch test
def _b_block(n_bytes):
    return plain((97, 98, 99), [2] + run_digits(n_bytes - 3) + [3, 2])


for _level in (1, 9):
    for _n in (100000, 100001):
        case("B-level%d-%d-bytes" % (_level, _n), lambda n=_n: _b_block(n), "ok" if _n <= 100000 * _level else "size:1663", level=_level)

case("B-level1-run-past-100000-bytes", lambda: plain((97, 98, 99), [2] + run_digits(100000) + [3]), "run-size:1647", level=1)
case("B-level9-run-past-100000-bytes", lambda: plain((97, 98, 99), [2] + run_digits(100000) + [3]), level=9)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = "USLTCMB"
