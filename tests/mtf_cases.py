"""Blocks for the MTF / RLE2 stage built from what the stage is made of: a sequence of run heads, each with an MTF rank and a run
length (test_gpu_mtf_tiers.py: ranks only, every run of length one; test_gpu_mtf_runs.py: both).

Beside the generator stands a plain restatement of the stage's output from the construction alone (`expected_from_heads`): the
oracle's MTF is the reference's serial walk over the bytes, the restatement says what a case was built to contain, and the
tests hold the two against each other before anything is compared with the GPU.
"""
import numpy as np

RUNA, RUNB = 0, 1


def _alphabet(asz):
    """asz byte values, ascending, 0 and 255 among them (when asz >= 2)"""
    return [0] if asz == 1 else sorted(set(int(round(i * 255.0 / (asz - 1))) for i in range(asz)))


def block_from_heads(asz, ranks, lens, first_rank0=False):
    """Bytes whose i-th run head has MTF rank ranks[i] and run length lens[i] >= 1.  Every rank is in 1 .. asz-1, except that with
    first_rank0 head 0 has rank 0: it is the smallest byte value of the alphabet, the only head that can stand at the front of
    the list it meets.  Symbols of the alphabet the ranks never reach are appended as runs of length one at the end, so that the
    block does have `asz` symbols; returns (bytes, the ranks of ALL heads, the lengths of ALL heads, the closing ones included)."""
    syms = _alphabet(asz)
    assert len(syms) == asz and len(ranks) == len(lens)
    lst = list(syms)
    seen = set()
    out = []
    all_ranks = []
    for i, r in enumerate(ranks):
        assert (r == 0 and i == 0) if (first_rank0 and i == 0) else 1 <= r < asz, (i, r)
        s = lst.pop(r)
        lst.insert(0, s)
        out.append(s)
        seen.add(s)
        all_ranks.append(r)
    for s in syms:
        if s not in seen:
            r = lst.index(s)
            if r == 0:          # only when no rank was asked for at all: the lone first head
                assert not out
            lst.pop(r)
            lst.insert(0, s)
            out.append(s)
            all_ranks.append(r)
    all_lens = np.ones(len(out), dtype=np.int64)
    all_lens[:len(lens)] = np.asarray(lens, dtype=np.int64)
    assert all_lens.min() >= 1
    U = np.repeat(np.asarray(out, dtype=np.uint8), all_lens)
    return U, np.asarray(all_ranks, dtype=np.int64), all_lens


def heads_from_ranks(asz, ranks):
    """Bytes whose i-th run head has MTF rank ranks[i] (every rank in 1 .. asz-1; runs of length one).  Symbols of the alphabet
    the ranks never reach are appended once each at the end, so that the block does have `asz` symbols; returns (bytes, the
    ranks of ALL heads, the closing ones included)."""
    U, all_ranks, _ = block_from_heads(asz, ranks, [1] * len(ranks))
    return U, all_ranks


def heads_of(U):
    """a block of bytes read back into heads: (asz, ranks, lens, positions), by a plain move-to-front over its run heads"""
    U = np.asarray(U, dtype=np.uint8)
    pos = np.flatnonzero(np.concatenate([[True], U[1:] != U[:-1]]))
    lens = np.diff(np.append(pos, U.size))
    lst = np.unique(U).tolist()
    asz = len(lst)
    ranks = []
    for s in U[pos].tolist():
        r = lst.index(s)
        ranks.append(r)
        lst.insert(0, lst.pop(r))
    return asz, np.asarray(ranks, dtype=np.int64), lens.astype(np.int64), pos


def zero_runs(ranks, lens):
    """the zero-run length behind every head: the whole run for a head of rank 0, the run without its head otherwise"""
    ranks, lens = np.asarray(ranks, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    return lens - (ranks > 0)


def run_digits(z):
    """bijective base-2 digits of a zero-run length z >= 1, low digit first: RUNA counts 1 and RUNB 2 at weight 2^i"""
    out = []
    z = int(z)
    while z > 0:
        if z & 1:
            out.append(RUNA)
            z = (z - 1) >> 1
        else:
            out.append(RUNB)
            z = (z - 2) >> 1
    return out


def expected_from_heads(U, asz, ranks, lens):
    """what the stage must emit for a block built by block_from_heads, from the construction alone: (A with the end-of-block
    symbol, freq[asz + 2], alist, nheads)"""
    A = []
    for r, z in zip(np.asarray(ranks).tolist(), zero_runs(ranks, lens).tolist()):
        if r > 0:
            A.append(r + 1)
        if z:
            A.extend(run_digits(z))
    A.append(asz + 1)
    A = np.asarray(A, dtype=np.uint16)
    freq = np.bincount(A, minlength=asz + 2).astype(np.uint32)
    alist = np.unique(np.asarray(U, dtype=np.uint8))
    assert alist.size == asz and int(np.sum(lens)) == np.asarray(U).size
    return A, freq, alist, len(ranks)
