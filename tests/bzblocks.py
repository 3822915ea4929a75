"""Bzip2 streams whose blocks hold exactly the bytes a test chooses (no tests in here: test_bzblocks_host.py, test_gpu_dec_backend.py).

A block of a .bz2 stream carries the bytes `tt` the Huffman stage decodes and a start index `origPtr`.  The reference's decoder
(J/Bzip2_joined_.js:1677-1753) sorts `tt` stably, walks the permutation from `dbuf[origPtr]` for `count` steps -- the bytes it
visits are called `w` here -- and expands `w` by the RLE1 rule while it walks.  `walk` and `expand` restate those two loops in
plain Python: they are the specification the decoders are held to.  `stream_from_blocks` wraps chosen `w` arrays into a valid
stream with the oracle's encoder stages (its cyclic BWT, MTF/RLE2 and block packer), `stream_from_tt` does the same for a raw
`tt` / `origPtr` pair that need not be the BWT of anything.  The case tables at the end are shared by the CPU and the GPU tests.
"""
import numpy as np

SPL = 64                      # the decoder's splitter spacing (csrc/decode_dev.h)
TILE = 16384                  # bytes of w per RLE1 tile (UR_TILE)


# ---------------------------------------------------------------- the reference's two loops
def expand(w, previous=None):
    """the output loop (:1732-1753) over the visited bytes `w`; `previous`: the byte decoded by hand in front of the loop
    (:1697-1701; the last byte of w for a cyclic BWT)"""
    w = bytes(bytearray(w))
    out = bytearray()
    if not w:
        return bytes(out)
    current = w[-1] if previous is None else previous
    run = -1
    for byte in w:
        previous = current
        current = byte
        if run == 3:                 # run++ === 3: this byte is a count
            copies = current
            outbyte = previous
            current = -1
        else:
            copies = 1
            outbyte = current
        run += 1
        out += bytes([outbyte]) * copies
        if current != previous:
            run = 0
    return bytes(out)


def walk(tt, orig):
    """the inverse BWT (:1679-1702, :1735-1737): (w, visited slots, start).  Slot j of the stable counting sort of tt points at
    the index of the j-th smallest byte; the walk starts on the slot dbuf[orig] points at and makes len(tt) steps."""
    tt = np.ascontiguousarray(tt, dtype=np.uint8)
    nxt = np.argsort(tt, kind="stable").tolist()
    low = tt.tolist()
    start = nxt[orig]
    pos, slots, w = start, [], bytearray()
    for _ in range(tt.size):
        slots.append(pos)
        w.append(low[pos])
        pos = nxt[pos]
    return np.frombuffer(bytes(w), dtype=np.uint8), np.array(slots, dtype=np.int64), start


def cycle_length(slots, start):
    """steps until the walk stands on `start` again (len(slots) if it does not come back within the block)"""
    again = np.nonzero(np.asarray(slots)[1:] == start)[0]
    return int(again[0]) + 1 if again.size else len(slots)


def stretch_lengths(slots, start):
    """lengths of the walks between splitters (slot % 64 == 0, or the start slot) along the cycle through the start"""
    cyc = np.asarray(slots)[: cycle_length(slots, start)]
    marks = np.nonzero((cyc % SPL == 0) | (cyc == start))[0].tolist()
    return [b - a for a, b in zip(marks, marks[1:] + [cyc.size])]


# ---------------------------------------------------------------- streams
def _bits(value, n):
    return np.array([(value >> (n - 1 - i)) & 1 for i in range(n)], dtype=np.uint8)


def _block_bits(oracle, tt, orig, out_bytes):
    tt = np.ascontiguousarray(tt, dtype=np.uint8)
    A, _, asz = oracle.mtf_rle2(tt, tt)
    crc = oracle.crc32(np.frombuffer(out_bytes, dtype=np.uint8))
    rc, arr, nbits = oracle.bzip2_block_bits(A, asz, np.unique(tt), crc, orig)
    assert rc == 0, rc
    return np.unpackbits(arr)[:nbits], crc


def _assemble(level, blocks):
    """blocks: (bits, crc) each -> the stream: BZh<level>, the blocks bit by bit, the end magic, the combined CRC"""
    parts = [np.unpackbits(np.frombuffer(b"BZh%d" % level, dtype=np.uint8))]
    combined = 0
    for bits, crc in blocks:
        parts.append(bits)
        combined = (((combined << 1) | (combined >> 31)) & 0xFFFFFFFF) ^ crc
    parts += [_bits(0x177245385090, 48), _bits(combined, 32)]
    return np.packbits(np.concatenate(parts))


def stream_from_blocks(oracle, blocks, level=9):
    """every block: the bytes w the decoder's walk is to visit (1 .. 100000 * level of them) -> (stream, expected output)"""
    packed, want = [], []
    for w in blocks:
        w = np.ascontiguousarray(w, dtype=np.uint8)
        assert 1 <= w.size <= 100000 * level
        out = expand(w)
        tt, pidx = oracle.bwt_cyclic(w)
        packed.append(_block_bits(oracle, tt, pidx, out))
        want.append(out)
    return _assemble(level, packed), b"".join(want)


def stream_from_tt(oracle, tt, orig, level=9):
    """one block that holds the decoded bytes `tt` and the start index `orig` as they are -> (stream, expected output)"""
    tt = np.ascontiguousarray(tt, dtype=np.uint8)
    assert 1 <= tt.size <= 100000 * level and 0 <= orig < tt.size
    out = expand(walk(tt, orig)[0], previous=int(tt[orig]))
    return _assemble(level, [_block_bits(oracle, tt, orig, out)]), out


# ---------------------------------------------------------------- pieces of the cases
def lit(n, phase=0):
    """n bytes without two equal neighbours (values 0 .. 250)"""
    return ((np.arange(phase, phase + n, dtype=np.int64) * 7 + 1) % 251).astype(np.uint8)


def _put(w, at, piece):
    """`piece` into w at `at`; the neighbours are made to differ from the piece's ends (253 is in no piece and no background)"""
    piece = np.asarray(piece, dtype=np.uint8)
    w[at: at + piece.size] = piece
    if at > 0 and w[at - 1] == piece[0]:
        w[at - 1] = 253
    if at + piece.size < w.size and w[at + piece.size] == piece[-1]:
        w[at + piece.size] = 253
    return w


def dense_runs(seed, n, high=False):
    """runs of geometric length (mean 3) of bytes from {0, 1, 2, 3} (high: and {254, 255}): count bytes equal run bytes throughout"""
    rng = np.random.RandomState(seed)
    alphabet = np.array([0, 1, 2, 3, 254, 255] if high else [0, 1, 2, 3], dtype=np.uint8)
    lengths = rng.geometric(1.0 / 3.0, size=n)
    values = alphabet[rng.randint(0, alphabet.size, size=n)]
    return np.repeat(values, lengths)[:n].copy()


def page_input(seed, page_len, copies, low):
    """`copies` x (a random page of bytes below 100 + a terminator of its own, 128 ..); copy `low` has the smallest terminator.
    The sorted rotations come in groups of `copies` rows, ordered by terminator inside a group: with 64 or 128 copies the rows of
    copy `low` are the splitters, and what the walk visits outside that copy is one stretch."""
    page = np.random.RandomState(seed).randint(0, 100, size=page_len).astype(np.uint8)
    return np.concatenate([np.concatenate([page, [128 + (c - low) % copies]]).astype(np.uint8) for c in range(copies)])


def periodic_input(p, n):
    """a unit of p bytes (no period of its own) repeated and cut to n bytes"""
    unit = {1: [97], 2: [97, 98], 3: [97, 98, 99]}.get(p)
    if unit is None:
        unit = np.random.RandomState(900 + p).randint(0, 200, size=p)
    unit = np.asarray(unit, dtype=np.uint8)
    return np.tile(unit, n // p + 1)[:n].copy()


class Case:
    """name, family ('R1' .. 'W4'), make() -> ('blocks', [w, ...]) or ('tt', tt, orig), and what the CPU test asserts about it"""

    def __init__(self, name, make, **claims):
        self.name, self.family, self.make, self.claims = name, name.split("-")[0], make, claims


_streams = {}


def stream(oracle, case):
    """(stream, expected output) of a case; built once per process"""
    if case.name not in _streams:
        made = case.make()
        _streams[case.name] = stream_from_blocks(oracle, made[1]) if made[0] == "blocks" else stream_from_tt(oracle, made[1], made[2])
    return _streams[case.name]


def first_difference(got, want):
    """a message for a failed comparison: sizes and the first differing offset"""
    got, want = np.frombuffer(bytes(got), dtype=np.uint8), np.frombuffer(bytes(want), dtype=np.uint8)
    m = min(got.size, want.size)
    bad = np.nonzero(got[:m] != want[:m])[0]
    at = int(bad[0]) if bad.size else m
    return "sizes %d / %d, first difference at offset %d (got %s, want %s)" % (
        got.size, want.size, at, got[at: at + 8].tolist(), want[at: at + 8].tolist())


# ---------------------------------------------------------------- family R: RLE1 expansion (blocks given as w)
R1_BORDERS, R1_SHIFTS, R1_COUNTS = (16, 1024, 16384, 32768), range(-5, 2), (0, 1, 3, 251, 255)


def _r1(B, d, run_byte, count):
    def make():
        w = lit(B + 64)
        return "blocks", [_put(w, B + d - 4, [run_byte] * 4 + [count])]          # the run ends at B + d - 1, its count byte is w[B + d]
    return make


def _r2(v, n, lead):
    def make():
        if lead is None:
            return "blocks", [np.full(n, v, dtype=np.uint8)]
        w = lit(20 + lead + n + 50)                                              # 20 + lead bytes of text in front: the stretch starts at lead mod 5
        return "blocks", [_put(w, 20 + lead, np.full(n, v, dtype=np.uint8))]
    return make


def _r3(L, before):
    def make():
        return "blocks", [_put(lit(TILE + 64), TILE - before, [2] * L)]         # `before` bytes of the stretch in the first tile
    return make


def _r4_cases():
    a = 9
    cases = []
    for k in (1, 2, 3, 4):                       # (four equal bytes and no count byte behind them: no encoder emits this)
        cases.append(("ends-after-%d-equal" % k, np.concatenate([lit(300), [252] * k])))
    for c in (0, 255):
        cases.append(("ends-in-count-%d" % c, np.concatenate([lit(300), [252] * 4, [c]])))
    cases.append(("first-three-equal-last", np.concatenate([[a] * 3, lit(300, 2), [a]])))        # run = -1: the byte decoded by hand is no part of a run
    cases.append(("first-four-equal-last", np.concatenate([[a] * 4, [6], lit(300, 2), [a]])))
    for n in (1, 2, 4, 5):
        cases.append(("len-%d-equal" % n, np.full(n, 3)))
        cases.append(("len-%d-distinct" % n, lit(n, 5)))
    return [(name, np.asarray(w, dtype=np.uint8)) for name, w in cases]


# R5: a tile of 16384 bytes of w whose expansion is exactly `size` bytes: literals and 33 runs of four bytes 252 with a count byte,
# 32 of them 255 and one chosen.  In tile 0: 16384 - 33 + 32 * 255 + c = 24511 + c.  In tile 1 behind a tile that ends in four
# bytes 253, its first byte their count byte 10: 10 + 16383 - 33 + 32 * 255 + c = 24520 + c.
R5_SIZES = (24575, 24576, 24577)
R5_COUNTS = {("tile0", 24575): 64, ("tile0", 24576): 65, ("tile0", 24577): 66, ("tile1", 24575): 55, ("tile1", 24576): 56, ("tile1", 24577): 57}


def _r5(where, size):
    def make():
        tile = lit(TILE, 3)
        for i in range(33):
            _put(tile, 100 + 400 * i, [252] * 4 + [255 if i < 32 else R5_COUNTS[(where, size)]])
        if where == "tile0":
            return "blocks", [np.concatenate([tile, lit(3000)])]
        front = _put(lit(TILE), TILE - 4, [253] * 4)
        tile[0] = 10
        return "blocks", [np.concatenate([front, tile, lit(3000)])]
    return make


def _r6_first_block(k):
    """a block that expands to k bytes (1 .. 15)"""
    return lit(k, 11) if k <= 4 else np.array([9, 9, 9, 9, k - 4], dtype=np.uint8)


def _r_cases():
    out = []
    for B in R1_BORDERS:
        for d in R1_SHIFTS:
            for c in R1_COUNTS:
                out.append(Case("R1-B%d-d%+d-count%d" % (B, d, c), _r1(B, d, 252, c), out_len=B + 64 - 1 + c))
            out.append(Case("R1-B%d-d%+d-run7x11" % (B, d), _r1(B, d, 7, 7), out_len=B + 64 - 1 + 7))
            out.append(Case("R1-B%d-d%+d-run255x259" % (B, d), _r1(B, d, 255, 255), out_len=B + 64 - 1 + 255))
    for v in (0, 1, 4, 5, 255):
        for n in (16383, 16384, 16385, 16388, 32769, 50000):
            out.append(Case("R2-v%d-n%d" % (v, n), _r2(v, n, None)))
            for lead in range(5):
                out.append(Case("R2-v%d-n%d-lead%d" % (v, n, lead), _r2(v, n, lead)))
    for L in range(4, 15):
        for before in range(1, L):
            out.append(Case("R3-len%d-before%d" % (L, before), _r3(L, before)))
    for name, w in _r4_cases():
        out.append(Case("R4-" + name, lambda w=w: ("blocks", [w])))
    for where in ("tile0", "tile1"):
        for size in R5_SIZES:
            out.append(Case("R5-%s-%d" % (where, size), _r5(where, size), tile=0 if where == "tile0" else 1, tile_out=size))
    out.append(Case("R5-maximal", lambda: ("blocks", [np.tile(np.array([7, 7, 7, 7, 255], dtype=np.uint8), 3277)]), out_len=848743))
    out.append(Case("R6-17-blocks", lambda: ("blocks", [dense_runs(600 + k, 4096 + k, high=k % 3 == 0) for k in range(17)])))
    for k in range(16):                          # (no block expands to 0 bytes: for k = 0 the large block is the stream's first)
        out.append(Case("R6-first-block-out%d" % k,
                        lambda k=k: ("blocks", ([_r6_first_block(k)] if k else []) + [dense_runs(700 + k, 20000, high=k % 3 == 0)])))
    for seed in range(24):
        out.append(Case("R7-seed%d" % seed, lambda seed=seed: ("blocks", [dense_runs(seed, 40000 + seed, high=seed % 3 == 0)])))
    return out


# ---------------------------------------------------------------- family W: the inverse BWT's walk
# W1 (seed, page bytes, copies, copy with the smallest terminator), found by a search over these on the CPU; the stretches above
# 2 steps that each gives (test_bzblocks_host.py asserts them): a page of P bytes in 64 copies with the splitters' copy second
# makes one stretch of exactly P steps from the start to that copy and one of 62 P + 64 behind it.
W1_PAGES = (
    ((1, 1000, 64, 0), {63064: 1}),                      # start % 64 == 0: the start entry is an alias
    ((1, 383, 64, 1), {383: 1, 23810: 1}),
    ((1, 384, 64, 1), {384: 1, 23872: 1}),
    ((1, 385, 64, 1), {385: 1, 23934: 1}),
    ((1, 767, 64, 1), {767: 1, 47618: 1}),
    ((1, 768, 64, 1), {768: 1, 47680: 1}),
    ((1, 769, 64, 1), {769: 1, 47742: 1}),
    ((1, 383, 128, 1), {383: 1, 23810: 1, 24193: 1}),
    ((1, 500, 63, 0), None),                             # copies that do not line up with the splitters: many short stretches
    ((1, 500, 65, 3), None),
    ((1, 300, 96, 2), None),
)
# W2 (block length, seed of four-letter text, start slot), found by a search over seeds on the CPU
W2_TEXTS = ((50, 14, 0), (50, 0, 36), (4096, 27, 192), (4096, 0, 3339), (1000, 20, 704), (1000, 0, 821))
W3_PERIODS = (1, 2, 3, 63, 64, 65, 383, 384, 385, 1000)
W4_LENGTHS = (1, 2, 63, 64, 65, 4097, 20000, 100000)


def four_letter_text(seed, n):
    return (np.random.RandomState(seed).randint(0, 4, n) + 97).astype(np.uint8)


def _w4(n, alphabet):
    rng = np.random.RandomState(4000 + n + alphabet)
    tt = rng.randint(0, alphabet, n).astype(np.uint8)
    return tt, sorted({int(rng.randint(0, n)), 0, n - 1})


def _w_cases():
    out = []
    for (seed, page, copies, low), stretches in W1_PAGES:
        out.append(Case("W1-page%d-x%d-low%d" % (page, copies, low),
                        lambda a=(seed, page, copies, low): ("blocks", [page_input(*a)]), stretches=stretches, alias=(low == 0 and copies == 64)))
    for n, seed, start in W2_TEXTS:
        out.append(Case("W2-n%d-seed%d" % (n, seed), lambda n=n, seed=seed: ("blocks", [four_letter_text(seed, n)]), start=start))
    for p in W3_PERIODS:
        whole = p * -(-20000 // p)
        out.append(Case("W3-p%d-n%d" % (p, whole), lambda p=p, n=whole: ("blocks", [periodic_input(p, n)]), cycle=p))
        if p > 1:                                # (every length is a multiple of 1)
            out.append(Case("W3-p%d-n%d" % (p, whole + 1), lambda p=p, n=whole + 1: ("blocks", [periodic_input(p, n)]), cycle=whole + 1))
    for n in W4_LENGTHS:
        for alphabet in (3, 256):
            for orig in _w4(n, alphabet)[1]:
                out.append(Case("W4-n%d-of%d-orig%d" % (n, alphabet, orig), lambda n=n, a=alphabet, orig=orig: ("tt", _w4(n, a)[0], orig)))
    out.append(Case("W4-one-value", lambda: ("tt", np.full(5000, 7, dtype=np.uint8), 1234), cycle=1))
    return out


R_CASES = _r_cases()
W_CASES = _w_cases()
CASES = R_CASES + W_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SENTINEL_CASES = [c for c in W_CASES if c.family in ("W1", "W3")]            # W5: the same bytes through the sentinel form (BWTC)
