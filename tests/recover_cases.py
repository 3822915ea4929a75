"""Bzip2 recovery (cjs_bzip2_recover): the ctypes binding, a model of the contract and the damaged inputs the tests use (no tests in
here: test_recover_host.py checks the model and the inputs on the CPU, test_gpu_recover.py holds the GPU to them).

The model restates include/cjs_hip.h with the oracle: every position of the 48-bit block magic (numpy), each decoded by
Oracle.bzip2_decompress_block on a copy of the input that starts with 'BZh9' (the level-9 limits, the block CRC checked), where the
block ends by a parse of its bit string (`block_end`), the selection rule, and both result forms put together bit by bit."""
import ctypes
import hashlib
import os
import sys

import numpy as np

import bzblocks
import recipes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u8p = ctypes.POINTER(ctypes.c_uint8)
S = ctypes.c_size_t
V = ctypes.c_void_p
MAGIC_BLOCK, MAGIC_END = 0x314159265359, 0x177245385090
SHADOWED = 1
EMPTY_STREAM = b"BZh9" + MAGIC_END.to_bytes(6, "big") + bytes(4)


class Found(ctypes.Structure):
    _fields_ = [("bitpos", ctypes.c_uint64), ("end_bit", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("size", ctypes.c_uint32),
                ("status", ctypes.c_int32), ("crc", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def bind(path):
    try:
        import torch  # noqa: F401  (first, as the package does: torch brings a HIP runtime of its own, and the process must have one)
    except Exception:
        pass
    L = ctypes.CDLL(path)
    PF, PL = ctypes.POINTER(Found), ctypes.POINTER(ctypes.c_long)
    L.cjs_bzip2_recover.argtypes = [u8p, S, ctypes.c_int, ctypes.POINTER(u8p), ctypes.POINTER(S), PF, ctypes.c_long, PL, V]
    L.cjs_bzip2_recover.restype = ctypes.c_int
    L.cjs_bzip2_recover_device.argtypes = [V, S, ctypes.c_int, V, S, ctypes.POINTER(S), PF, ctypes.c_long, PL, V]
    L.cjs_bzip2_recover_device.restype = ctypes.c_int
    L.cjs_bzip2_decompress.argtypes = [u8p, S, ctypes.c_int, ctypes.POINTER(u8p), ctypes.POINTER(S), V]
    L.cjs_bzip2_table.argtypes = [u8p, S, ctypes.c_int, V, V, ctypes.c_long, V]
    L.cjs_bzip2_table.restype = ctypes.c_long
    L.cjs_free.argtypes = [V]
    L.cjs_free.restype = None
    return L


def u8(x):
    return np.frombuffer(bytes(x), dtype=np.uint8).copy() if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8)


def as_tuples(found, n):
    return [(f.bitpos, f.end_bit, f.out_off, f.size, f.status, f.crc) for f in found[:n]]


# ---------------------------------------------------------------- the model
def magics(buf, magic=MAGIC_BLOCK):
    """every bit position at which the 48 bits of `magic` start"""
    bits = np.unpackbits(u8(buf))
    if bits.size < 48:
        return []
    hit = np.ones(bits.size - 47, dtype=bool)
    for i in range(48):
        hit &= bits[i: bits.size - 47 + i] == ((magic >> (47 - i)) & 1)
    return np.nonzero(hit)[0].tolist()


def _peek20(bits):
    """for every bit position the next 20 bits as a number (zeros behind the end)"""
    pad = np.concatenate([bits, np.zeros(20, np.uint8)]).astype(np.uint32)
    v = np.zeros(bits.size, dtype=np.uint32)
    for k in range(20):
        v |= pad[k: k + bits.size] << (19 - k)
    return v.tolist()


_ends = {}      # first 256 bits of a block -> [(length in bits, sha256 of the bit string)]: a block parsed once is known again


def block_end(bits, peek, p):
    """first bit behind the end-of-block code of the block whose magic starts at bit p -- a block the oracle has accepted, so no
    error paths: header, used map, selectors, code lengths, then the Huffman symbols up to the end-of-block symbol"""
    key = bits[p: p + 256].tobytes()
    for length, digest in _ends.get(key, ()):
        if hashlib.sha256(bits[p: p + length].tobytes()).digest() == digest:
            return p + length
    b = bits.tolist() if bits.size < (1 << 16) else None

    def get(pos, k):
        v = 0
        for x in (b[pos: pos + k] if b is not None else bits[pos: pos + k].tolist()):
            v = (v << 1) | x
        return v
    pos = p + 48 + 32 + 1 + 24
    top = get(pos, 16); pos += 16
    used = 0
    for i in range(16):
        if top & (1 << (15 - i)):
            used += bin(get(pos, 16)).count("1"); pos += 16
    groups = get(pos, 3); pos += 3
    nsel = get(pos, 15); pos += 15
    order, sel = list(range(groups)), []
    for _ in range(nsel):
        j = 0
        while get(pos, 1):
            pos += 1; j += 1
        pos += 1
        order.insert(0, order.pop(j))
        sel.append(order[0])
    nsym, tabs = used + 2, []
    for _ in range(groups):
        t = get(pos, 5); pos += 5
        lens = []
        for _ in range(nsym):
            while get(pos, 1):
                t += 1 if get(pos + 1, 1) == 0 else -1
                pos += 2
            pos += 1
            lens.append(t)
        maxlen = max(lens)
        tab = np.zeros(1 << maxlen, dtype=np.uint16)      # prefix of maxlen bits -> code length | end of block << 8
        code = 0
        for ln in range(min(lens), maxlen + 1):
            for s in range(nsym):
                if lens[s] == ln:
                    tab[code << (maxlen - ln): (code + 1) << (maxlen - ln)] = ln | (256 if s == nsym - 1 else 0)
                    code += 1
            code <<= 1
        tabs.append((tab.tolist(), 20 - maxlen))
    for g in sel:
        tab, sh = tabs[g]
        for _ in range(50):
            e = tab[peek[pos] >> sh]
            assert e & 255, "no code at bit %d" % pos
            pos += e & 255
            if e & 256:
                _ends.setdefault(key, []).append((pos - p, hashlib.sha256(bits[p: pos].tobytes()).digest()))
                return pos
    raise AssertionError("no end of block")


def _num(bits, pos, k):
    v = 0
    for x in bits[pos: pos + k].tolist():
        v = (v << 1) | x
    return v


class Model:
    """hits: every block magic; recovered: (bitpos, end_bit, decoded bytes, stored crc) of the recovered blocks; shadowed: the hits
    inside a recovered block; data / stream: the two result forms"""


def model(oracle, buf):
    buf = u8(buf)
    m = Model()
    m.hits = magics(buf)
    bits = np.unpackbits(buf)
    as9 = buf.copy()
    as9[:4] = np.frombuffer(b"BZh9", dtype=np.uint8)[: min(4, buf.size)]
    peek = None
    m.recovered, m.shadowed, last_end = [], [], 0
    for p in m.hits:
        if p < last_end:
            m.shadowed.append(p)
            continue
        rc, data = oracle.bzip2_decompress_block(as9, p)
        if rc != 0:
            continue
        if peek is None:
            peek = _peek20(bits)
        end = block_end(bits, peek, p)
        if end >= bits.size:                                   # touches the end: counts as cut off
            continue
        m.recovered.append((p, end, data.tobytes(), _num(bits, p + 48, 32)))
        last_end = end
    m.data = b"".join(r[2] for r in m.recovered)
    m.stream = bzblocks._assemble(9, [(bits[p:e], crc) for p, e, _, crc in m.recovered]).tobytes()
    return m


# ---------------------------------------------------------------- the inputs
_made = {}


def _once(name, make):
    if name not in _made:
        _made[name] = make()
    return _made[name]


def compress(oracle, data, level):
    rc, s = oracle.bzip2_compress(data, level)
    assert rc == 0
    return s


def text250():
    return _once("text250", lambda: recipes.textgen(250000, 7))


def stream250(oracle):
    """textgen(250000, 7) at level 1: 96108 bytes, blocks at bits 32, 299452, 604689 of 99898, 99897, 50205 bytes"""
    return _once("stream250", lambda: compress(oracle, text250(), 1))


BLOCKS250 = [(32, 99898), (299452, 99897), (604689, 50205)]
EOS250 = 768778


def stream250_l9(oracle):
    return _once("stream250_l9", lambda: compress(oracle, text250(), 9))


def members(oracle):
    """three member streams of levels 1, 5 and 9, and their payloads"""
    def make():
        parts = [recipes.textgen(150000, 11), recipes.textgen(60000, 12), recipes.textgen(30001, 13)]
        return np.concatenate([compress(oracle, d, lv) for d, lv in zip(parts, (1, 5, 9))]), b"".join(d.tobytes() for d in parts)
    return _once("members", make)


def flip(buf, bit):
    out = u8(buf).copy()
    out[bit >> 3] ^= 0x80 >> (bit & 7)
    return out


def damage_a(oracle):
    return flip(stream250(oracle), (299452 + 604689) // 2)


def damage_b(oracle):
    return flip(stream250(oracle), 299452 + 53)


def damage_c(oracle):
    s = np.delete(stream250(oracle), ((32 + 299452) // 2) >> 3)
    s[:4] = 0
    return s[:-2000].copy()


def damage_d(oracle):
    return np.concatenate([stream250(oracle), u8(b"garbage!"), compress(oracle, text250()[:1000], 9)])


def shifted(oracle, k):
    """the whole file k bits later: k one-bits in front"""
    return np.packbits(np.concatenate([np.ones(k, np.uint8), np.unpackbits(stream250(oracle))]))


def forty(oracle):
    """40 blocks of 1 .. 40 bytes: (stream, output, [(bitpos, size)])"""
    def make():
        s, want = bzblocks.stream_from_blocks(oracle, [bzblocks.lit(k, 3 * k) for k in range(1, 41)])
        rc, tab = oracle.bzip2_table(s, 0)
        assert rc == 0 and len(tab) == 40
        return s, want, tab
    return _once("forty", make)


FORTY_DAMAGE = {"every-third": list(range(2, 40, 3)), "first": [0], "last": [39], "all": list(range(40)), "none": []}


def forty_damaged(oracle, which):
    """the stored CRC (bit p + 53) of the blocks FORTY_DAMAGE[which] flipped -> (stream, the bytes of the others)"""
    s, want, tab = forty(oracle)
    out, keep, off = s.copy(), [], 0
    for k, (p, size) in enumerate(tab):
        if k in FORTY_DAMAGE[which]:
            out = flip(out, p + 53)
        else:
            keep.append(want[off: off + size])
        off += size
    return out, b"".join(keep)


MAP_VALUES = [0x21, 0x23, 0x24, 0x27, 0x2a, 0x2d, 0x2e, 0x31, 0x33, 0x36, 0x37, 0x39, 0x3b, 0x3c, 0x3f, 0x70, 0x90, 0xf0]


def magic_in_map(oracle):
    """3000 bytes whose used-byte map spells the block magic: (level-9 stream, the bytes); magics at bits 32 and 137, one block"""
    def make():
        vals = np.array(MAP_VALUES, dtype=np.uint8)
        steps = np.random.RandomState(41).randint(1, vals.size, 3000 - vals.size)      # (no byte twice in a row: a run's count byte would join the map)
        idx = np.concatenate([np.arange(vals.size), (vals.size - 1 + np.cumsum(steps)) % vals.size])
        data = vals[idx]
        assert (data[1:] != data[:-1]).all()
        return compress(oracle, data, 9), data.tobytes()
    return _once("magic_in_map", make)


def level_limit(oracle):
    """one block of more BWT bytes than level 1 allows behind a 'BZh1' header: (stream, the bytes)"""
    def make():
        data = recipes.textgen(140831, 5)
        s = compress(oracle, data, 9).copy()
        s[3] = ord("1")
        return s, data.tobytes()
    return _once("level_limit", make)


def random_damage(oracle, seed):
    """one to three of: a bit flipped, a byte deleted, a byte inserted, a span of 16 bytes zeroed"""
    rng = np.random.RandomState(7000 + seed)
    s = stream250(oracle).copy()
    for _ in range(int(rng.randint(1, 4))):
        kind, at = int(rng.randint(0, 4)), int(rng.randint(0, s.size - 16))
        if kind == 0:
            s = flip(s, at * 8 + int(rng.randint(0, 8)))
        elif kind == 1:
            s = np.delete(s, at)
        elif kind == 2:
            s = np.insert(s, at, np.uint8(rng.randint(0, 256)))
        else:
            s[at: at + 16] = 0
    return np.ascontiguousarray(s)


SEEDS = list(range(24))


# ---------------------------------------------------------------- the calls
def recover_host(L, buf, as_stream, cap=4096):
    """-> (rc, bytes, found tuples)"""
    a = u8(buf)
    keep = a if a.size else np.zeros(1, np.uint8)
    out, n, nf = u8p(), S(0), ctypes.c_long(0)
    found = (Found * cap)()
    rc = L.cjs_bzip2_recover(keep.ctypes.data_as(u8p), a.size, 1 if as_stream else 0, ctypes.byref(out), ctypes.byref(n), found, cap, ctypes.byref(nf), None)
    if rc:
        return rc, b"", []
    assert nf.value <= cap
    data = ctypes.string_at(out, n.value) if n.value else b""
    L.cjs_free(out)
    return 0, data, as_tuples(found, nf.value)


def recover_device(L, buf, as_stream, cap_bytes=None, in_shift=1, out_shift=3, cap=4096):
    """d_in at byte in_shift of a tensor, d_out at byte out_shift of a 0xA5-filled one with cap_bytes for the call and 64 guard bytes
    behind them, which must stay as they are -> (rc, bytes, found tuples, out_n)"""
    import torch
    a = u8(buf)
    src = torch.from_numpy(np.concatenate([np.zeros(in_shift, np.uint8), a, np.full(7, 0x5A, np.uint8)])).cuda()
    if cap_bytes is None:
        cap_bytes = 4 * text250().size
    dst = torch.full((out_shift + cap_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n, nf = S(0), ctypes.c_long(0)
    found = (Found * cap)()
    rc = L.cjs_bzip2_recover_device(src.data_ptr() + in_shift, a.size, 1 if as_stream else 0, (dst.data_ptr() + out_shift) if cap_bytes else None, cap_bytes,
                                    ctypes.byref(n), found, cap, ctypes.byref(nf), None)
    torch.cuda.synchronize()
    whole = dst.cpu().numpy()
    assert (whole[:out_shift] == 0xA5).all() and (whole[out_shift + cap_bytes:] == 0xA5).all(), "bytes outside d_out[0, out_cap) were written"
    data = whole[out_shift: out_shift + n.value].tobytes() if rc == 0 else b""
    return rc, data, as_tuples(found, nf.value) if rc in (0, -33) else [], n.value


def digest(L, oracle, with_device):
    """cases 1-3 through both forms -> {name: sha256 of (bytes, found)}: what a child process with shrunk batches compares"""
    inputs = {"stream250": stream250(oracle), "stream250_l9": stream250_l9(oracle), "empty": u8(EMPTY_STREAM), "members": members(oracle)[0],
              "a": damage_a(oracle), "b": damage_b(oracle), "c": damage_c(oracle), "d": damage_d(oracle), "shift13": shifted(oracle, 13)}
    for which in FORTY_DAMAGE:
        inputs["forty-" + which] = forty_damaged(oracle, which)[0]
    out = {}
    for name, buf in sorted(inputs.items()):
        for as_stream in (0, 1):
            rc, data, found = recover_host(L, buf, as_stream)
            out["%s/%d/host" % (name, as_stream)] = hashlib.sha256(repr((rc, data, found)).encode()).hexdigest()
            if with_device:
                rc, data, found, _ = recover_device(L, buf, as_stream)
                out["%s/%d/device" % (name, as_stream)] = hashlib.sha256(repr((rc, data, found)).encode()).hexdigest()
    return out


if __name__ == "__main__":      # the child process of test_gpu_recover.py's batch test: the digests as one JSON line
    import json
    import support
    sys.path.insert(0, ROOT)
    print(json.dumps(digest(bind(os.path.join(support.PKG, "libcjs_hip.so")), support.Oracle(), True)))
