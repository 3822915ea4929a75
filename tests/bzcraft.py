"""Bzip2 blocks written bit by bit, and a model of the reference's block reader (no tests in here: test_bzcraft_host.py,
test_gpu_crafted_headers.py; the cases are in bzcraft_cases.py).

`block` writes what no compressor emits: any used map, raw unary selector values (a value equal to the table count, or one above
it), any `n_sel`, code lengths whose delta string zig-zags or is given bit by bit, tables that are over- or under-subscribed.
It returns the bits with the bit offset of every section, so that a test can prove what a case claims about them.  `stream`
frames blocks into a .bz2 stream.  `model` restates the reference's sequential reader (J/Bzip2_joined_.js:1440-1670) in plain
Python and gets the bytes from `bzblocks.walk` / `bzblocks.expand`: it is the specification the decoders are held to, and where
the block CRCs of the crafted streams come from (never from the code under test).
"""
import numpy as np

import bzblocks

RUNA, RUNB = 0, 1
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090
STRETCH = 2048                # bits the decoder's header wave reads at a time: 64 lanes x 32 bits (csrc/bz_stage2.h)
DATA_ERROR, OBSOLETE_INPUT = -5, -7


class NoCode(Exception):
    """the table has no code that decodes to this symbol"""


def _u32(x):
    return x & 0xFFFFFFFF


def _i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


# ---------------------------------------------------------------- the reference's rules, shared by the writer and the model
def unmtf_selectors(values, group_count):
    """:1481-1493: the list has 256 slots, zero-initialised, the first group_count hold 0 .. group_count - 1"""
    lst = [0] * 256
    for i in range(group_count):
        lst[i] = i
    out = []
    for j in values:
        src = lst[j]
        for i in range(j, 0, -1):
            lst[i] = lst[i - 1]
        lst[0] = src
        out.append(src)
    return out


class Table:
    """:1522-1580: permute / limit / base of one code-length list.  limit and base are unsigned 32-bit, permute is zero-initialised."""

    def __init__(self, length):
        n = len(length)
        mn = mx = length[0]
        for i in range(1, n):
            if length[i] > mx:
                mx = length[i]
            elif length[i] < mn:
                mn = length[i]
        self.min_len, self.max_len = mn, mx
        self.permute, self.limit, self.base = [0] * 258, [0] * 22, [0] * 21
        temp = [0] * 21
        pp = 0
        for i in range(mn, mx + 1):
            for t in range(n):
                if length[t] == i:
                    self.permute[pp] = t
                    pp += 1
        for i in range(n):
            temp[length[i]] = (temp[length[i]] + 1) & 0xFFFF
        pp = t = 0
        for i in range(mn, mx):
            pp += temp[i]
            self.limit[i] = _u32(pp - 1)
            pp = _i32(pp << 1)
            t += temp[i]
            self.base[i + 1] = _u32(pp - t)
        self.limit[mx + 1] = 0                     # (the sentinel, a double, stored into 32 bits)
        self.limit[mx] = _u32(pp + temp[mx] - 1)
        self.base[mn] = 0
        self.length = list(length)
        self._codes = {}

    def decode(self, get):
        """:1605-1616: (symbol, None) or (None, name of the failed check); get(n) reads n bits"""
        i = self.min_len
        j = get(i)
        while True:
            if i > self.max_len:
                return None, "no-code:1608"
            if j <= self.limit[i]:
                break
            j = (j << 1) | get(1)
            i += 1
        j -= self.base[i]
        if j < 0 or j >= 258:
            return None, "index:1615"
        return self.permute[j], None

    def code(self, sym):
        """the bits (a str) that decode to `sym`, the canonical code by (length, symbol); NoCode if the decode rule gives none"""
        if sym not in self._codes:
            i = self.length[sym]
            at = [p for p in range(len(self.length)) if self.permute[p] == sym and self.length[self.permute[p]] == i][0]
            j = at + self.base[i]                  # (the slot the symbol has in permute, undone)
            bits = None
            if j < (1 << i):
                bits = format(j, "0%db" % i)
                it = iter(bits)
                read = []

                def get(n):
                    v = 0
                    for _ in range(n):
                        b = next(it, None)
                        read.append(b)
                        v = (v << 1) | int(b or 0)
                    return v
                got, _ = self.decode(get)
                if got != sym or len(read) != i or None in read:
                    bits = None
            self._codes[sym] = bits
        if self._codes[sym] is None:
            raise NoCode("symbol %d (length %d) of %r" % (sym, self.length[sym], self.length))
        return self._codes[sym]


# ---------------------------------------------------------------- the writer
def delta_string(lengths, zig=0, start=None):
    """:1506-1520 backwards: 5 bits, then per symbol '10' = one longer, '11' = one shorter, closed by '0'; zig: that many
    up/down pairs (down/up at 20) in front of every terminator (a list: per symbol)"""
    cur = lengths[0] if start is None else start
    out = [format(cur, "05b")]
    for s, ln in enumerate(lengths):
        while cur < ln:
            out.append("10")
            cur += 1
        while cur > ln:
            out.append("11")
            cur -= 1
        out.append(("1110" if cur == 20 else "1011") * (zig if isinstance(zig, int) else zig[s]))
        out.append("0")
    return "".join(out)


class Block:
    """bits: uint8 array of 0 / 1 (the CRC field, bits 48 .. 79, is zero until `stream` fills it); the offsets are bit offsets
    from the block's magic: sel = (first, end) of the selector list, tab[t] = (5-bit start, first delta bit, end) of table t,
    groups[i] = first bit of group i's codes, end = the bit behind the last code written"""

    def __init__(self, bits, sel, tab, groups, end, sel_tables, crc):
        self.bits, self.sel, self.tab, self.groups, self.end, self.sel_tables, self.crc = bits, sel, tab, groups, end, sel_tables, crc

    def text(self, a, b):
        return "".join("01"[x] for x in self.bits[a:b])

    def lane_words(self, origin, end):
        """the 32-bit words the 64 lanes read from a section's stretch origin on, as strings (the last one may be short)"""
        s = self.text(origin, end)
        return [s[i: i + 32] for i in range(0, len(s), 32)]


def block(used=(), tables=(), selectors=(), symbols=(), n_sel=None, group_count=None, orig=0, empty_rows=(), randomised=0, eob=True,
          crc=None, tail=""):
    """one block.  used: the used bytes; empty_rows: rows (0 .. 15) whose coarse bit is set over a fine word of 0.  tables: one
    dict(lengths=[..], zig=0, start=None, raw=None) each (raw: the table's whole string, start value included, as written).
    selectors: the unary values as written; n_sel / group_count as written (default: how many there are).  symbols: RUNA, RUNB,
    rank symbols 2 .., or a str of bits written as they are (one code of its group); eob: append the end-of-block symbol.
    Group i is coded with the table the reference's rule gives for selector i.  tail: bits behind the last code."""
    used = sorted(set(used))
    n_used = len(used)
    out = [format(BLOCK_MAGIC, "048b"), "0" * 32, "1" if randomised else "0", format(orig, "024b")]
    coarse, fine = 0, [0] * 16
    for u in used:
        coarse |= 0x8000 >> (u >> 4)
        fine[u >> 4] |= 0x8000 >> (u & 15)
    for r in empty_rows:
        assert fine[r] == 0
        coarse |= 0x8000 >> r
    out.append(format(coarse, "016b"))
    for r in range(16):
        if coarse & (0x8000 >> r):
            out.append(format(fine[r], "016b"))
    count = len(tables) if group_count is None else group_count
    out.append(format(count, "03b"))
    out.append(format(len(selectors) if n_sel is None else n_sel, "015b"))
    at = sum(len(x) for x in out)
    sel_text = "".join("1" * v + "0" for v in selectors)
    sel = (at, at + len(sel_text))
    out.append(sel_text)
    at = sel[1]
    tab, coders = [], []
    for t in tables:
        s = t["raw"] if t.get("raw") is not None else delta_string(t["lengths"], t.get("zig", 0), t.get("start"))
        tab.append((at, at + 5, at + len(s)))
        at += len(s)
        out.append(s)
        coders.append(Table(t["lengths"]) if t.get("lengths") is not None else None)
    syms = list(symbols) + ([n_used + 1] if eob else [])
    sel_tables = unmtf_selectors([min(v, count) for v in selectors], count)      # (a value above the count: the block is rejected there)
    groups = []
    for i, s in enumerate(syms):
        if i % 50 == 0:
            groups.append(at)
            assert i // 50 < len(sel_tables), "more groups than (valid) selectors"
        piece = s if isinstance(s, str) else coders[sel_tables[i // 50]].code(s)
        out.append(piece)
        at += len(piece)
    out.append(tail)
    bits = np.frombuffer("".join(out).encode(), dtype=np.uint8) - 48
    return Block(bits, sel, tab, groups, at, sel_tables, crc)


def _bits_of(value, n):
    return np.frombuffer(format(value, "0%db" % n).encode(), dtype=np.uint8) - 48


def stream(blocks, level=9, tail=b""):
    """BZh<level>, the blocks, the end magic, the combined CRC; tail: bytes behind the stream.  A block's CRC is its own `crc`, or
    that of the bytes the model gives for it (0 if the model rejects it)."""
    parts = [np.unpackbits(np.frombuffer(b"BZh%d" % level, dtype=np.uint8))]
    combined = 0
    for b in blocks:
        crc = b.crc
        if crc is None:
            got = read_block(_Reader(b.bits.tolist(), 80), 100000 * level)
            crc = _crc(_bytes_of(*got)) if not isinstance(got, str) else 0
        bits = b.bits.copy()
        bits[48:80] = _bits_of(crc, 32)
        parts.append(bits)
        combined = _u32((combined << 1) | (combined >> 31)) ^ crc
    parts += [_bits_of(END_MAGIC, 48), _bits_of(combined, 32)]
    return np.concatenate([np.packbits(np.concatenate(parts)), np.frombuffer(tail, dtype=np.uint8)])


# ---------------------------------------------------------------- the model
_oracle = None


def _crc(data):
    global _oracle
    if _oracle is None:
        import support
        _oracle = support.Oracle()
    return _oracle.crc32(np.frombuffer(bytes(data), dtype=np.uint8))


class _Reader:
    """bits past the end read as zeros (:147-151)"""

    def __init__(self, bits, pos=0):
        self.bits, self.n, self.pos = bits, len(bits), pos

    def get(self, n):
        v = 0
        for _ in range(n):
            v <<= 1
            if self.pos < self.n:
                v |= self.bits[self.pos]
                self.pos += 1
        return v


def read_block(r, dbuf_size):
    """:1446-1677 from the randomised bit on: (tt, orig), or the name of the check that fails with its line"""
    if r.get(1):
        return "randomised:1446"
    orig = r.get(24)
    if orig > dbuf_size:
        return "orig:1449"
    t = r.get(16)
    sym_to_byte, sym_total = [0] * 256, 0
    for i in range(16):
        if t & (1 << (15 - i)):
            k = r.get(16)
            for j in range(16):
                if k & (1 << (15 - j)):
                    sym_to_byte[sym_total] = i * 16 + j
                    sym_total += 1
    group_count = r.get(3)
    if group_count < 2 or group_count > 6:
        return "group-count:1471"
    n_sel = r.get(15)
    if n_sel == 0:
        return "n-sel:1478"
    values = []
    for i in range(n_sel):
        j = 0
        while r.get(1):
            if j >= group_count:
                return "selector:1490"
            j += 1
        values.append(j)
    selectors = unmtf_selectors(values, group_count)
    sym_count = sym_total + 2
    groups = []
    for j in range(group_count):
        length = [0] * sym_count
        t = r.get(5)
        for i in range(sym_count):
            while True:
                if t < 1 or t > 20:
                    return "length:1509"
                if not r.get(1):
                    break
                if not r.get(1):
                    t += 1
                else:
                    t -= 1
            length[i] = t
        groups.append(Table(length))
    mtf = list(range(256))
    run_pos = t = 0
    dbuf = bytearray()
    selector = 0
    left = 0
    while True:
        if not left:
            left = 50
            if selector >= n_sel:
                return "selectors-run-out:1601"
            huf = groups[selectors[selector]]
            selector += 1
        left -= 1
        sym, bad = huf.decode(r.get)
        if bad:
            return bad
        if sym == RUNA or sym == RUNB:
            if not run_pos:
                run_pos, t = 1, 0
            t += run_pos if sym == RUNA else 2 * run_pos
            run_pos = _i32(run_pos << 1)           # the weight is an int32: the 32nd digit makes it 0 and the run is forgotten
            continue
        if run_pos:
            run_pos = 0
            if len(dbuf) + t > dbuf_size:
                return "run-size:1647"
            dbuf += bytes([sym_to_byte[mtf[0]]]) * max(t, 0)
        if sym > sym_total:
            break
        if len(dbuf) >= dbuf_size:
            return "size:1663"
        uc = mtf.pop(sym - 1)
        mtf.insert(0, uc)
        dbuf.append(sym_to_byte[uc])
    if orig >= len(dbuf):
        return "orig:1677"
    return np.frombuffer(bytes(dbuf), dtype=np.uint8), orig


def _bytes_of(tt, orig):
    return bzblocks.expand(bzblocks.walk(tt, orig)[0], previous=int(tt[orig]))


def model(data):
    """the bytes of a (single) stream, or the name of the check that fails (:1408-1450, :1756, :1782)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if data.size < 4 or bytes(data[:3]) != b"BZh" or not 1 <= int(data[3]) - 48 <= 9:
        return "magic:1413"
    dbuf_size = 100000 * (int(data[3]) - 48)
    r = _Reader(np.unpackbits(data).tolist(), 32)
    out, combined = [], 0
    while True:
        if (r.pos + 7) // 8 >= data.size:          # (:1777: the input is at its end)
            break
        h = r.get(48)
        if h == END_MAGIC:
            if r.get(32) != combined:
                return "stream-crc:1782"
            break
        if h != BLOCK_MAGIC:
            return "magic:1438"
        target = r.get(32)
        combined = _u32((combined << 1) | (combined >> 31)) ^ target
        got = read_block(r, dbuf_size)
        if isinstance(got, str):
            return got
        piece = _bytes_of(*got)
        if _crc(piece) != target:
            return "block-crc:1756"
        out.append(piece)
    return b"".join(out)


def status_of(result):
    """the code the decoders give for a model result"""
    if not isinstance(result, str):
        return 0
    return OBSOLETE_INPUT if result.startswith("randomised") else DATA_ERROR
