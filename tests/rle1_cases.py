"""Inputs and block capacities for stage 0 (RLE1, block boundaries, block CRCs) with the capacity as a free argument
(test_gpu_rle1_cap.py, test_gpu_rle1_batch.py), and what each family claims to contain.

The product only ever passes cap = level * 100000 - 19, one block boundary per 100 KB.  A small cap turns an input of a few tiles
into thousands of boundaries, each at another chunk phase, subtile offset and run position.  Beside the generators stands a plain
numpy model of the chunk rule per byte (`Model`) and, from it and the oracle's blocks alone, the facts about every block
(`block_facts`): where its last byte lies in its run, whether its count byte was dropped, whether the next block starts inside a
run.  tests/test_rle1_cases_host.py asserts on the CPU that every family contains what it says before anything goes to the GPU.
"""
import functools

import numpy as np

import recipes

RT = 4096                     # input tile of the stage-0 kernels
SC = 1024                     # tiles per chunk of the three-phase tile scans
WIN = 16384                   # window of rle_probe (and of the CRC ranges)
NSPEC = 32                    # boundaries speculated per round of the walk
CAP_FLOOR = 2                 # cjs_stage_rle1_cap refuses smaller ones (max_blocks_for divides by cap * 4 / 5)

RUNLENS = [2, 3, 4, 5, 6, 7, 8] + list(range(254, 262)) + list(range(509, 516)) + [1020, 5000]
CAPS_SMALL = list(range(CAP_FLOOR, 13))
CAPS_255 = list(range(254, 262))
CAPS_1275 = list(range(1274, 1282))
CAPS_4096 = list(range(4093, 4102))
CAPS_MOD5_1 = [16, 21, 2001, 9981, 19981]            # == 1 (mod 5), like every level * 100000 - 19


# ------------------------------------------------------------------ bytes
@functools.lru_cache(maxsize=None)
def _pool(seed=0x51ED, n=90000):
    return recipes.xorshift_bytes(n, seed, 63, 32)        # values 32 .. 95: the planted runs use bytes above


def noise(n, off=0):
    """n bytes of xorshift noise (mask 63, add 32), from offset `off` of one shared pool (repeated when n is larger)"""
    p = _pool()
    off %= p.size
    if off + n <= p.size:
        return p[off: off + n].copy()
    return np.resize(np.concatenate([p[off:], p[:off]]), n)


def runfree(n, off=0):
    """n bytes of the same noise with every byte that equals its predecessor taken out: no run at all, RLE1 length n"""
    a = noise(min(n + n // 16 + 64, _pool().size), off)
    a = a[np.concatenate([[True], a[1:] != a[:-1]])]
    if a.size < n:                                       # longer than the pool: repeat, then mend the seams
        a = np.resize(a, n + n // 16 + 64)
        a = a[np.concatenate([[True], a[1:] != a[:-1]])]
    assert a.size >= n
    return a[:n].copy()


def run(byte, n):
    return np.full(n, byte, dtype=np.uint8)


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts])


# ------------------------------------------------------------------ the chunk rule per byte, in plain numpy
def emitted_fresh(m):
    """output bytes of the first m bytes of one run chunked from its first byte: five per whole chunk of 255, then up to four
    literals, the fourth bringing the count byte with it"""
    m = np.asarray(m, dtype=np.int64)
    return 5 * (m // 255) + np.where(m % 255 < 4, m % 255, 5)


class Model:
    """Per byte of `data`, counted from the start of its maximal run: rs / re = the run's first index and the index behind its
    last, dp = offset in its chunk of 255, c = bytes it puts out (1, 1, 1, 2, then 0), G = exclusive prefix of c (N + 1 entries)"""

    def __init__(self, data):
        a = self.a = np.ascontiguousarray(data, dtype=np.uint8)
        n = self.n = a.size
        idx = np.arange(n, dtype=np.int64)
        head = np.ones(n, dtype=bool)
        head[1:] = a[1:] != a[:-1]
        self.head = head
        self.rs = np.maximum.accumulate(np.where(head, idx, 0))
        ends = np.nonzero(head)[0][1:]
        self.re = np.concatenate([ends, [n]])[np.cumsum(head) - 1] if n else idx
        self.dp = (idx - self.rs) % 255
        self.c = np.where(self.dp < 3, 1, np.where(self.dp == 3, 2, 0)).astype(np.int64)
        self.G = np.concatenate([[0], np.cumsum(self.c)])

    def trailing_run(self):
        return int(self.n - self.rs[-1]) if self.n else 0


def block_facts(m, blocks, cap):
    """From the oracle's blocks [(bytes, crc, s, e)] and the model, per block: S, E, L (RLE1 length); inrun = the block starts
    inside a run (its first byte equals the one in front); r_end = end of that run (S where it starts on a run boundary);
    emitted = what the block's input puts out when the run it starts in is chunked afresh from S and everything behind as the
    model has it (L, or L + 1 when the block was cut between a fourth equal byte and its count); dp_last = chunk offset of the
    block's last input byte under that chunking; cont = the next block starts inside the run of this block's last byte."""
    a, n = m.a, m.n
    S = np.array([b[2] for b in blocks], dtype=np.int64)
    E = np.array([b[3] for b in blocks], dtype=np.int64)
    L = np.array([b[0].size for b in blocks], dtype=np.int64)
    f = {"S": S, "E": E, "L": L, "cap": cap}
    if not len(blocks):
        return f
    assert S[0] == 0 and E[-1] == n and np.array_equal(S[1:], E[:-1]) and np.all(E > S)
    inrun = (S > 0) & (a[S] == a[np.maximum(S - 1, 0)])
    r_end = np.where(inrun, m.re[S], S)
    first_end = np.minimum(r_end, E)
    pe = E - 1
    f["inrun"], f["r_end"] = inrun, r_end
    f["emitted"] = emitted_fresh(first_end - S) + (m.G[E] - m.G[first_end])
    f["dp_last"] = np.where(pe < r_end, (pe - S) % 255, m.dp[pe])
    f["runlen_last"] = m.re[pe] - m.rs[pe]
    f["cont"] = (E < n) & (a[np.minimum(E, n - 1)] == a[pe])
    f["full"] = L == cap
    return f


def check_model(f):
    """the model and the oracle agree on every block's length: a full block put out cap bytes, or cap + 1 with its last input
    byte a fourth equal byte whose count was dropped; the last block what is left"""
    if not len(f["S"]):
        return
    cap, L, em = f["cap"], f["L"], f["emitted"]
    assert np.all(L[:-1] == cap) and 0 < L[-1] <= cap
    cut = em == L + 1
    assert np.all((em == L) | cut), "model and oracle differ on a block's length"
    assert np.all(~cut | ((f["dp_last"] == 3) & (L == cap)))


def boundary_tags(m, f):
    """what the block ends and block starts of one (input, cap) hit: a set of names (see FAMILY_A_NEEDS)"""
    t = set()
    if not len(f["S"]):
        return t
    S, E, L, cap = f["S"], f["E"], f["L"], f["cap"]
    full, dp, cont = f["full"], f["dp_last"], f["cont"]
    if np.any(full & (f["runlen_last"] == 1)):
        t.add("end_on_literal")
    for d in range(4):
        if np.any(full & (f["runlen_last"] >= 4) & (dp == d)):
            t.add("end_at_chunk_offset_%d" % d)
    if np.any(full & (dp == 3) & (f["emitted"] == cap + 1) & cont):
        t.add("count_dropped_next_in_run")
    if np.any(full & (dp == 3) & (f["emitted"] == cap) & cont):
        t.add("count_is_last_byte")
    # block starts inside a run
    inr = f["inrun"]
    rl = m.re[S] - m.rs[S]                                  # whole length of the run a block starts in
    left = np.minimum(S - 1 - m.rs[S], 2)                   # equal bytes in front of the previous block's last byte (probe: <= 2)
    right = 1 + np.minimum(m.re[S] - S - 1, 2)              # the block's first byte and up to two more
    short = inr & (rl <= 3)
    if np.any(short & (left > 0)):
        t.add("short_run_left_probe")
    if np.any(short & (right > 1)):
        t.add("short_run_right_probe")
    if np.any(inr & (rl >= 4) & (1 + left + right > 3)):
        t.add("unclean_by_probe")
    if np.any(inr & (m.re[S] - S >= 4)):
        t.add("start_in_run_4_more")
    # three blocks in a row filled inside one run: blocks k, k+1, k+2 start inside it and k+2 ends inside it
    if S.size >= 3:
        k = np.arange(S.size - 2)
        same = inr[k] & (E[k + 2] <= m.re[S[k]]) & full[k] & full[k + 1] & full[k + 2]
        if np.any(same):
            t.add("three_blocks_in_one_run")
        if np.any(same & (cap % 5 == 0)):
            t.add("fill_in_run_cap_multiple_of_5")
    if inr[-1] and m.re[S[-1]] == m.n and L[-1] < cap:
        t.add("last_block_is_run_tail")
    return t


FAMILY_A_NEEDS = {
    "end_on_literal", "end_at_chunk_offset_0", "end_at_chunk_offset_1", "end_at_chunk_offset_2", "end_at_chunk_offset_3",
    "count_dropped_next_in_run", "count_is_last_byte", "short_run_left_probe", "short_run_right_probe", "start_in_run_4_more",
    "three_blocks_in_one_run", "fill_in_run_cap_multiple_of_5", "last_block_is_run_tail",
}


# ------------------------------------------------------------------ family A: boundary phases
def planted(gaps, lens, off=0, tail=None):
    """noise with one run of lens[i] behind gap i (gaps cycle), run bytes 0x61 .. 0x67 in turn (above every noise byte, never
    the same twice in a row); `tail`: a last run that reaches the end of the input"""
    parts, o = [], off
    for i, L in enumerate(lens):
        g = gaps[i % len(gaps)]
        parts += [noise(g, o), run(0x61 + i % 7, L)]
        o += g
    if tail:
        parts += [noise(gaps[0], o), run(0x7A, tail)]
    return cat(*parts)


@functools.lru_cache(maxsize=None)
def inputs():
    """the named inputs of families A, D, E and F, built once"""
    d = {}
    d["a_small"] = planted([157, 220, 311, 393, 470], RUNLENS, 0, tail=1020)                      # ~21 KB
    d["a_large"] = planted([301, 655, 1009, 1490, 777, 512], RUNLENS + RUNLENS[::-1], 7000, tail=5000)   # ~65 KB
    d["two_sym"] = recipes.xorshift_bytes(20000, 4242, 1, 48)
    # D: runs that straddle tile ends, one of them with its fourth byte in front of the tile end and more than 251 bytes behind
    d["d_tiles"] = cat(noise(8192 - 50, 100), run(0x61, 100), noise(12288 - 100 - 8242, 9000), run(0x62, 600),
                       noise(20480 - 3 - 12788, 20000), run(0x63, 9), noise(61440 - 20486, 30000))
    return d


def family_a():
    """[(input name, cap)]"""
    return ([("a_small", c) for c in CAPS_SMALL] + [("two_sym", c) for c in CAPS_SMALL + CAPS_255] +
            [("a_large", c) for c in CAPS_255 + CAPS_1275 + CAPS_4096 + CAPS_MOD5_1])


# ------------------------------------------------------------------ family B: rounds of the speculation, end of input
B_CAP = 50


@functools.lru_cache(maxsize=None)
def family_b():
    """{name: (data, cap)}.  `rounds`: 75 clean boundaries, a boundary behind the third byte of a run of 40, 40 more clean ones.  totals_K_X: run-free
    noise of K * cap + X bytes (RLE1 length the same), X in 0, 1.  dropped_count_at_eof: the last block fills with the fourth
    equal byte as the input's last byte."""
    cap = B_CAP
    d = {"rounds": (cat(runfree(75 * cap + 47, 11), run(0x7A, 40), runfree(40 * cap + 17, 5000)), cap)}
    for k in (31, 32, 33, 64):
        for x in (0, 1):
            d["totals_%d_%d" % (k, x)] = (runfree(k * cap + x, 100 * k + x), cap)
    d["dropped_count_at_eof"] = (cat(runfree(33 * cap - 4, 77), run(0x7A, 4)), cap)
    return d


def clean_flags(m, f):
    """per block: its end is what the walk calls a clean boundary (the cap-th byte came out with the block's last input byte, no
    count byte hangs over, and the next block starts a run or lies in a run of at most three bytes)"""
    E, n = f["E"], m.n
    nxt = np.minimum(E, n - 1)
    fresh = (E >= n) | (m.a[nxt] != m.a[E - 1]) | (m.re[nxt] - m.rs[nxt] <= 3)
    return f["full"] & (f["emitted"] == f["cap"]) & fresh


# ------------------------------------------------------------------ family C: geometry
@functools.lru_cache(maxsize=None)
def family_c(oracle_len):
    """{name: (data, cap)}; oracle_len(data) = RLE1 length of data as one block (places a boundary behind a noise prefix)"""
    d = {}
    rf = runfree(20000, 333)
    for c in CAPS_255 + CAPS_4096:
        d["offsets_%d" % c] = (rf, c)                      # run-free: block k ends at input offset (k + 1) * cap
    # a run of more than two tiles, a block start 4 chunks and 2 bytes into it: its tile holds no boundary behind the start
    pre = noise(3000, 1500)
    d["long_run_start_inside"] = (cat(pre, run(0x7A, 13000), noise(3000, 9)), oracle_len(pre) + 22)
    # a block start in the last subtile of tile 0 (offset 4003), its run of 200 ends in tile 1
    pre = noise(4000, 2500)
    d["start_in_last_subtile"] = (cat(pre, run(0x7A, 200), noise(5000, 60)), oracle_len(pre) + 3)
    return d


C_SEAM_N = 4 * 1024 * 1024 + 65536
C_SEAM_CAP = 99981
C_SEAM_RUNS = (3, 300, 9000)


@functools.lru_cache(maxsize=None)
def chunk_seam_input(L):
    """4 MiB + 64 KiB of noise with one run of L bytes that straddles byte 4 MiB (tile 1024, the first of the second chunk of
    the tile scans): a third of the run in front of it"""
    a = noise(C_SEAM_N, 0)
    seam = SC * RT
    s = seam - max(1, L // 3)
    a[s: s + L] = 0x7A
    return a


# ------------------------------------------------------------------ family D: the materialise kernel's fast path
D_CAPS = [11003, 16001, 20000, 27777, 39999]


def tile_facts(m, f, first=0):
    """rle_materialize's choice per input tile, restated: [(tile, block, fast, dst & 3, tot, head, off0 + tot)] for every whole
    tile, with `first` the first block of the rle1_finish window (rows are 256-aligned: dst = (block - first) * cap + off0)"""
    S, E, cap = f["S"], f["E"], f["cap"]
    out = []
    for t in range(m.n // RT):
        ts, te = t * RT, (t + 1) * RT
        k = int(np.searchsorted(E, ts, side="right"))      # first block with e > tile start
        s, e, r_end = int(S[k]), int(E[k]), int(f["r_end"][k])
        tot = int(m.G[te] - m.G[ts])
        off0 = int(emitted_fresh(r_end - s) + m.G[ts] - m.G[r_end]) if ts >= r_end else -1
        inside = ts >= s and ts >= r_end and te < e and te <= m.n
        fast = inside and off0 + tot + 1 < cap
        dst = ((k - first) * cap + off0) & 3
        head = min((4 - dst) & 3, tot)
        out.append({"tile": t, "block": k, "inside": inside, "fast": fast, "dst": dst, "tot": tot, "head": head, "end": off0 + tot})
    return out


def fast_path_tags(m, f):
    t = set()
    cap = f["cap"]
    for x in tile_facts(m, f):
        if x["fast"]:
            t.add("dst&3=%d" % x["dst"])
            t.add("tail&3=%d" % ((x["tot"] - x["head"]) & 3))
            if x["end"] == cap - 2:
                t.add("fast_ends_at_cap-2")
            if x["end"] == cap - 3:
                t.add("fast_ends_at_cap-3")
            ts, te = x["tile"] * RT, (x["tile"] + 1) * RT
            p = ts + np.nonzero((m.dp[ts:te] == 3) & (m.re[ts:te] > te))[0]      # count bytes whose run ends in a later tile
            follow = m.re[p] - (p + 1)
            if np.any(follow < 251):
                t.add("follow_from_next_tile")
            if np.any(follow > 251):
                t.add("follow_from_next_tile_clamped")
        elif x["inside"] and x["end"] == cap - 1:
            t.add("general_ends_at_cap-1")
    return t


FAMILY_D_NEEDS = ({"dst&3=%d" % i for i in range(4)} | {"tail&3=%d" % i for i in range(4)} |
                  {"fast_ends_at_cap-2", "fast_ends_at_cap-3", "general_ends_at_cap-1", "follow_from_next_tile",
                   "follow_from_next_tile_clamped"})


def family_d():
    """[(input name, cap)]: caps between 11 000 and 40 000, three of them 2, 1 and 3 bytes above what tile 3 of d_tiles has put
    out at its end (block 0 starts at 0, so a tile's output ends at G[tile end])"""
    m = Model(inputs()["d_tiles"])
    g = int(m.G[4 * RT])
    return [("d_tiles", c) for c in D_CAPS + [g + 2, g + 1, g + 3]] + [("a_large", c) for c in (11003, 16001)]


# ------------------------------------------------------------------ family E: ranged finish, used workspace
E_RANGES = (1, 2, 3, 7)
E_FILLS = (0x00, 0xFF)


def family_e():
    return [("a_small", 7), ("a_large", 257), ("a_large", 1276), ("a_large", 4099), ("a_large", 11003)]


# ------------------------------------------------------------------ family F: shares of the tile tables
F_WORLDS = (2, 3, 5, 8)


def tiles_per_rank(n, world):
    return (((n + RT - 1) // RT + world - 1) // world + 3) & ~3


@functools.lru_cache(maxsize=None)
def family_f():
    """{name: (data, [caps])}.  f_run: 64 tiles, a run of 100 000 bytes over the rank borders at 98 304, 131 072 and 163 840 (worlds
    2, 3, 5 and 8 all cut it).  f_exact: 40 tiles and 1234 bytes, run-free up to 99 000, so that block k ends at k * cap there: with
    world 2 (24 tiles per rank, border at byte 98 304) cap 12 288 ends block 7 with the last byte of rank 0's share and cap 19 661
    ends block 4 with the first byte of rank 1's; with world 8 the ranks 6 and 7 have no tile."""
    d = {}
    tail = planted([900, 450, 1200], RUNLENS * 3, 40000)
    d["f_run"] = (cat(noise(90000, 123), run(0x7A, 100000), tail[: 64 * RT - 190000]), [4099, 19981])
    d["f_exact"] = (cat(runfree(99000, 900), tail[: 40 * RT + 1234 - 99000]), [12288, 19661, 1277])
    assert d["f_run"][0].size == 64 * RT and d["f_exact"][0].size == 40 * RT + 1234
    return d


def probe_windows(m, world):
    """per rank: None without tiles, else (windows of 16 KiB rle_probe walks back from the share's first byte until it holds a
    run start, windows it walks forward from the share's end, the whole share lies inside one run)"""
    n = m.n
    tn, tpr = (n + RT - 1) // RT, tiles_per_rank(n, world)
    out = []
    for r in range(world):
        t0, t1 = r * tpr, min((r + 1) * tpr, tn)
        if t0 >= tn:
            out.append(None)
            continue
        lo, hi = t0 * RT, min(t1 * RT, n)
        back = (lo - 1 - int(m.rs[lo - 1])) // WIN + 1 if lo > 0 else 0
        fwd = 0
        if hi < n:
            nxt = hi if m.head[hi] else int(m.re[hi])                 # first run start at or behind hi (n: none)
            fwd = (nxt - hi) // WIN + 1 if nxt < n else (n - hi + WIN - 1) // WIN
        one_run = bool(lo > 0 and not m.head[lo] and int(m.re[lo]) >= hi)
        out.append((back, fwd, one_run))
    return out


# ------------------------------------------------------------------ family G: the batch kernels
G_CAP = 1000
G_TAILS = (3, 4, 5, 6, 255, 256, 259, 260)      # trailing runs: last byte at chunk offset 2, 3, 4, 5, 254, 0, 3, 4


@functools.lru_cache(maxsize=None)
def family_g():
    """(cap, [(name, bytes)]) in the order they are packed.  Every input is its own stream: runs and chunks restart at its
    first byte."""
    cap = G_CAP
    L = []
    for n in (1, 15, 16, 17, 4095, 4096, 4097, 8193):
        L.append(("len_%d" % n, planted([40, 333, 90], RUNLENS[:22], n)[:n]))
    # neighbours that would be one run of eight: 'zzz' ends one input, 'zzzzz' starts the next
    L.append(("ends_zzz", cat(noise(60, 1), run(0x7A, 3))))
    L.append(("starts_zzzzz", cat(run(0x7A, 5), noise(60, 2))))
    for x in (-1, 0, 1):
        L.append(("E_cap%+d_emits" % x, runfree(cap + x, 10 * (x + 2))))
        L.append(("E_cap%+d_absorbed" % x, cat(runfree(cap + x - 5, 10 * (x + 5)), run(0x7A, 9))))
    # a first run of R bytes, then run-free bytes: the block's cap-th byte comes out with input byte R - emitted(R) + cap - 1
    # (3161: byte 4095, the last of the block's first tile; 3162: byte 4096, the first of its second)
    for R in (3161, 3162):
        L.append(("block_ends_at_%d" % (R - int(emitted_fresh(R)) + cap - 1), cat(run(0x7A, R), runfree(2000, R))))
    L.append(("cut_before_count", cat(runfree(cap - 4, 4), run(0x7A, 8), runfree(700, 8))))
    L.append(("five_blocks", runfree(4 * cap + 300, 321)))
    # one block each, the last byte on both sides of the step from emitting (chunk offsets 0 .. 3) to absorbed (4 .. 254)
    for T in G_TAILS:
        L.append(("tail_run_%d" % T, cat(runfree(100 + T, T), run(0x7A, T))))
    L.append(("empty", np.zeros(0, dtype=np.uint8)))
    return cap, L


def pack(items, lead=1):
    """the inputs back to back behind `lead` bytes: (buffer, [(start, end)])"""
    se, off = [], lead
    for _, b in items:
        se.append((off, off + b.size))
        off += b.size
    buf = np.full(off, 0x7A, dtype=np.uint8)               # (the lead byte continues nothing either)
    for (s, e), (_, b) in zip(se, items):
        buf[s:e] = b
    return buf, se


def absorbed_flag(data):
    """the input's last byte goes into a count byte: it lies at offset >= 4 of a chunk of its trailing run of L bytes"""
    L = Model(data).trailing_run()
    return L > 0 and (L - 1) % 255 >= 4


# ------------------------------------------------------------------ family H: seeded sweep
H_SEED = 20261021
H_PAIRS = 200
H_CAPS = [2, 3, 4, 5, 6, 7, 9, 10, 12, 21, 254, 255, 256, 257, 258, 260, 261, 1274, 1276, 1280, 2001, 4093, 4096, 4097, 4101]


@functools.lru_cache(maxsize=None)
def family_h():
    """[(index, data, cap)]: inputs of 1 .. 8192 bytes, noise, two-symbol stretches and runs of RUNLENS in random order"""
    rng = np.random.RandomState(H_SEED)
    out = []
    for i in range(H_PAIRS):
        n = int(rng.randint(1, 8193))
        parts, have = [], 0
        while have < n:
            kind = rng.randint(0, 8)
            if kind < 4:
                p = noise(int(rng.randint(1, 400)), int(rng.randint(0, 80000)))
            elif kind == 4:
                p = noise(int(rng.randint(1, 300)), int(rng.randint(0, 80000))) & 1 | 0x30
            else:
                p = run(0x61 + int(rng.randint(0, 6)), RUNLENS[int(rng.randint(0, len(RUNLENS)))])
            parts.append(p)
            have += p.size
        out.append((i, cat(*parts)[:n], H_CAPS[int(rng.randint(0, len(H_CAPS)))]))
    return out


# ------------------------------------------------------------------ references, computed once and shared by the tests
_want, _model = {}, {}


def want(oracle, key, data, cap):
    """the oracle's blocks [(bytes, crc, s, e)] of (data, cap), kept under `key`"""
    k = (key, cap)
    if k not in _want:
        _want[k] = oracle.rle1_blocks_cap(data, cap)
    return _want[k]


def model(key, data):
    if key not in _model:
        _model[key] = Model(data)
    return _model[key]
