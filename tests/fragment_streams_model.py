"""Host model of fragment-level segmented framing
(onc_frame_fragment_streams) and of reassembly from scattered extents
(onc_defragment_extents), and the builders of the slabs their tests use
(tests/test_fragment_streams_model.py on the CPU,
tests/test_gpu_fragment_streams.py on the GPU).

Not a test file and not product code: the serial loop written in
include/onc_rpc.h in plain Python, and the concatenation definition of
onc_defragment_extents built on fragment_model.defragment. Expected values
come from here, from fragment_model and from the oracle's encoder, never from
the code under test.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

import fragment_model as FR
import streams_model as SM

OK, INCOMPLETE_MESSAGE, INCOMPLETE_HEADER, FRAGMENTED = 0, 1, 2, 3
KEEP = SM.KEEP     # marks the device chase keeps per segment (kernels.h kStreamKeep)
_BE = struct.Struct(">I")
EMPTY = _BE.pack(FR.LAST)          # an empty record: the bare last mark
CONT0 = _BE.pack(0)                # an empty continuation fragment


class Fragged:
    """What onc_frame_fragment_streams writes: frag_start u64[n], frag_len
    u32[n], frag_seg u32[n], rows u64[nseg, 8] and result u64[4]."""

    def __init__(self, start, length, seg, rows, result):
        self.frag_start = np.asarray(start, np.uint64)
        self.frag_len = np.asarray(length, np.uint32)
        self.frag_seg = np.asarray(seg, np.uint32)
        self.rows = np.asarray(rows, np.uint64).reshape(-1, 8)
        self.result = np.asarray(result, np.uint64)

    FIELDS = ("frag_start", "frag_len", "frag_seg", "rows", "result")

    def same(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.FIELDS)

    def diff(self, other):
        return [k for k in self.FIELDS if not np.array_equal(getattr(self, k), getattr(other, k))]


def walk(buf):
    """The walk of one segment: (recs, st, aux0, aux1) with recs = the complete
    records, each a list of (position, length) fragments; the pending run is
    dropped."""
    buf = bytes(buf)
    ln = len(buf)
    p, st, a0, a1 = 0, OK, 0, 0
    opened, recs = [], []
    while p < ln:
        left = ln - p
        if left < 4:
            st = INCOMPLETE_HEADER
            break
        h = _BE.unpack_from(buf, p)[0]
        want = (h & 0x7FFFFFFF) + 4
        if left < want:
            st, a0, a1 = INCOMPLETE_MESSAGE, left & 0xFFFFFFFF, want & 0xFFFFFFFF
            break
        opened.append((p, want))
        p += want
        if h >> 31:
            recs.append(opened)
            opened = []
    return recs, st, a0, a1


def frame_fragment_streams(slab, seg_off, seg_len, max_frags=None):
    """The serial loop of include/onc_rpc.h (max_frags None: unbounded)."""
    slab = bytes(slab)
    nseg = len(seg_off)
    cap = 1 << 62 if max_frags is None else int(max_frags)
    start, length, seg, rows = [], [], [], []
    if nseg == 0 or cap == 0:
        return Fragged(start, length, seg, np.zeros((nseg, 8), np.uint64), [0, 0, 0, 0])
    k = r = needed = stopped = 0
    full = False
    for s in range(nseg):
        o, ln = int(seg_off[s]), int(seg_len[s])
        recs, st, a0, a1 = walk(slab[o:o + ln])
        needed += sum(len(R) for R in recs)
        if full:
            rows.append((cap, 0, 0, OK, 0, 0, 0, 0))
            continue
        first, first_rec, consumed, cut = k, r, 0, False
        for R in recs:
            if len(R) > cap - k:
                cut = full = True
                break
            for fp, fl in R:
                start.append(o + fp)
                length.append(fl)
                seg.append(s)
                k += 1
            r += 1
            consumed = R[-1][0] + R[-1][1]
        row = (first, k - first, consumed, OK if cut else st, 0 if cut else a0, 0 if cut else a1, first_rec,
               r - first_rec)
        rows.append(row)
        stopped += row[3] != OK
    return Fragged(start, length, seg, rows, [k, needed, r, stopped])


def concat_extents(wire, frag_start, frag_len):
    """(C, frag_off): the extents' bytes back to back and their prefix sums."""
    wire = bytes(wire)
    parts = [wire[int(a):int(a) + int(n)] for a, n in zip(frag_start, frag_len)]
    off = np.concatenate(([0], np.cumsum([len(x) for x in parts]))).astype(np.uint64)
    return b"".join(parts), off


def defragment_extents(wire, frag_start, frag_len, out_cap=None):
    """onc_defragment_extents by its definition: fragment_model.defragment of
    the concatenation, result[1] = the fragments consumed."""
    C, off = concat_extents(wire, frag_start, frag_len)
    m = FR.defragment(C, off, out_cap)
    res = m["result"].copy()
    res[1] = len(frag_start) - int(res[3])
    m["result"] = res
    return m


# ---------------------------------------------------------------------------
# slabs
# ---------------------------------------------------------------------------
def record(rng, nfrag, max_body=40):
    """A record of nfrag fragments with random (some empty) bodies."""
    lens = rng.integers(0, max_body // max(nfrag, 1) + 2, nfrag)
    lens[rng.random(nfrag) < 0.2] = 0
    body = rng.bytes(int(lens.sum()))
    return FR.fragment(body, np.cumsum(lens)[:-1].tolist())


def ending(rng, kind):
    """What may follow a segment's complete records. -> (bytes, status, aux0, aux1)"""
    if kind == "clean":
        return b"", OK, 0, 0
    if kind == "pending":                       # fragments whose last one has not arrived
        return _pending(rng, int(rng.integers(1, 4))), OK, 0, 0
    if kind == "cut mark":                      # 1-3 bytes of a mark, behind 0-2 pending fragments
        n = int(rng.integers(1, 4))
        return _pending(rng, int(rng.integers(0, 3))) + b"\x80\x00\x00\x10"[:n], INCOMPLETE_HEADER, 0, 0
    if kind == "cut fragment":
        body = int(rng.integers(1, 30))
        have = int(rng.integers(0, body))
        last = FR.LAST if rng.random() < 0.5 else 0
        pre = _pending(rng, int(rng.integers(0, 3)))
        return pre + _BE.pack(last | body) + rng.bytes(have), INCOMPLETE_MESSAGE, 4 + have, 4 + body
    raise KeyError(kind)


def _pending(rng, k):
    """k continuation fragments (no last mark among them)."""
    return b"".join(_BE.pack(n) + rng.bytes(n) for n in rng.integers(0, 12, k).tolist())


ENDINGS = ("clean", "pending", "cut mark", "cut fragment")


@functools.lru_cache(maxsize=None)
def random_segments(nseg, seed=41):
    """nseg segments of 0-3 records of 1-5 fragments with random endings, at
    odd offsets. -> (slab, off, len)"""
    rng = np.random.default_rng(seed + nseg)
    sl = SM.Slab(front=int(rng.integers(0, 16)))
    for s in range(nseg):
        data = b"".join(record(rng, int(rng.integers(1, 6))) for _ in range(int(rng.integers(0, 4))))
        data += ending(rng, ENDINGS[int(rng.integers(0, 4))])[0]
        sl.add(data, gap=int(rng.integers(0, 20)))
    return sl.done()


# walked fragments per segment around the count the chase keeps; `last_at`:
# the (1-based) fragment carrying the segment's final last mark (0: none)
KEEP_CASES = ((KEEP - 1, KEEP - 1), (KEEP, KEEP), (KEEP + 1, KEEP + 1), (2 * KEEP, 2 * KEEP), (2 * KEEP + 1, 2 * KEEP + 1),
              (KEEP + 1, KEEP - 1), (KEEP + 1, KEEP), (2 * KEEP + 1, KEEP + 1), (2 * KEEP, KEEP), (20, 0))


def run_of(rng, walked, last_at, every=5):
    """`walked` fragments: last marks every `every` fragments up to fragment
    last_at, which has one; the rest is a pending run."""
    parts = []
    for i in range(1, walked + 1):
        n = int(rng.integers(0, 9))
        last = FR.LAST if i <= last_at and (i == last_at or i % every == 0) else 0
        parts.append(_BE.pack(last | n) + rng.bytes(n))
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def keep_slab(seed=43):
    """One segment per KEEP_CASES entry, a small healthy one between each."""
    rng = np.random.default_rng(seed)
    sl = SM.Slab(front=5)
    for i, (walked, last_at) in enumerate(KEEP_CASES):
        sl.add(run_of(rng, walked, last_at), gap=3 + i % 4)
        sl.add(record(rng, 2) + record(rng, 1), gap=i % 5)
    return sl.done()


@functools.lru_cache(maxsize=None)
def empties_slab():
    """Zero-length fragments, empty records and a record of only empty
    fragments, alone and mixed."""
    rng = np.random.default_rng(45)
    sl = SM.Slab(front=9)
    sl.add(EMPTY)
    sl.add(EMPTY * 3)
    sl.add(CONT0 * 4 + EMPTY)                                   # a record of five empty fragments
    sl.add(record(rng, 3) + CONT0 + CONT0 + EMPTY + EMPTY + FR.fragment(rng.bytes(9), [0, 0, 9]))
    sl.add(CONT0 * 3)                                           # pending empties only
    sl.add(EMPTY + CONT0)
    sl.add(b"")
    sl.add(CONT0 * 17 + EMPTY + EMPTY)                          # 18 fragments in the first record
    return sl.done()


@functools.lru_cache(maxsize=None)
def aligned_slab():
    """16 segments, one at each byte alignment of a 16-byte granule; the last
    one ends on the slab's last byte (the caller adds no padding)."""
    rng = np.random.default_rng(47)
    sl = SM.Slab(front=0)
    for a in range(16):
        pad = (a - sl.pos) % 16
        sl.parts.append((SM.GAP * 5)[:pad])
        sl.pos += pad
        sl.add(record(rng, 3) + record(rng, 1) + record(rng, 2), gap=4)
    slab, off, ln = sl.done()
    end = int(off[-1] + ln[-1])
    return slab[:end], off, ln


@functools.lru_cache(maxsize=None)
def capacity_slab():
    """Three segments, 12 fragments in complete records: records of 2, 3 | 4
    (then a pending run) | 1, 2 fragments."""
    rng = np.random.default_rng(49)
    sl = SM.Slab(front=3)
    sl.add(record(rng, 2) + record(rng, 3), gap=5)
    sl.add(record(rng, 4) + _pending(rng, 2), gap=2)
    sl.add(record(rng, 1) + record(rng, 2) + b"\x80\x00", gap=6)
    return sl.done()


@functools.lru_cache(maxsize=None)
def long_capacity_slab():
    """A segment of 40 fragments in records of 7 (the second chase), cut by
    the capacity, between two small ones."""
    rng = np.random.default_rng(51)
    sl = SM.Slab(front=1)
    sl.add(record(rng, 2), gap=4)
    sl.add(run_of(rng, 40, 35, every=7), gap=4)
    sl.add(record(rng, 3), gap=4)
    return sl.done()


# ---------------------------------------------------------------------------
# extents for onc_defragment_extents
# ---------------------------------------------------------------------------
def scatter(stream, order="ascending", gap=7, seed=53):
    """The fragments of a contiguous fragment stream laid out apart from each
    other in a new wire. -> (wire, frag_start, frag_len) in stream order;
    order: 'ascending' | 'descending' | 'shuffled' addresses."""
    stream = bytes(stream)
    fo = FR.frame_fragments(stream)[0].astype(np.int64)
    n = len(fo) - 1
    rng = np.random.default_rng(seed)
    place = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": rng.permutation(n)}[order]
    start = np.zeros(n, np.uint64)
    parts, pos = [], 0
    filler = SM.GAP * (gap // 4 + 2)
    for j in place:                                 # fragment j goes next in address order
        g = filler[:int(rng.integers(0, gap + 1))]
        parts.append(g)
        pos += len(g)
        start[j] = pos
        parts.append(stream[fo[j]:fo[j + 1]])
        pos += int(fo[j + 1] - fo[j])
    return b"".join(parts), start, np.diff(fo).astype(np.uint32)
