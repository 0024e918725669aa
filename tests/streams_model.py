"""Host model of segmented framing (onc_frame_streams) and the builders of
the slabs and segment lists its tests use (tests/test_streams_model.py on the
CPU, tests/test_gpu_streams.py and tests/test_gpu_extents.py on the GPU).

Not a test file and not product code: the serial loop written in
include/onc_rpc.h, in plain Python, checked against the oracle's
expected_message_len loop (oracle_ffi.frame_stream) run once per segment.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

import frame_model as FM

OK, INCOMPLETE_MESSAGE, INCOMPLETE_HEADER, FRAGMENTED = 0, 1, 2, 3
KEEP = 16          # record lengths the device chase keeps per segment (kernels.h kStreamKeep)
_BE = struct.Struct(">I")
# what lies between segments: bytes that read as the mark of a 28-byte record,
# so a framer that runs past a segment's end finds "records" there
GAP = bytes.fromhex("80000018")


class Framed:
    """What onc_frame_streams writes: rec_start u64[n], rec_len u32[n],
    rec_seg u32[n], rows u64[nseg, 6] and result u64[3]."""

    def __init__(self, start, length, seg, rows, result):
        self.rec_start = np.asarray(start, np.uint64)
        self.rec_len = np.asarray(length, np.uint32)
        self.rec_seg = np.asarray(seg, np.uint32)
        self.rows = np.asarray(rows, np.uint64).reshape(-1, 6)
        self.result = np.asarray(result, np.uint64)

    def same(self, other):
        return all(np.array_equal(getattr(self, k), getattr(other, k))
                   for k in ("rec_start", "rec_len", "rec_seg", "rows", "result"))


def frame_streams(slab, seg_off, seg_len, max_records=None):
    """The serial loop of include/onc_rpc.h (max_records None: unbounded)."""
    slab = bytes(slab)
    nseg = len(seg_off)
    cap = 1 << 62 if max_records is None else int(max_records)
    start, length, seg, rows = [], [], [], []
    if nseg == 0 or cap == 0:
        return Framed(start, length, seg, np.zeros((nseg, 6), np.uint64), [0, 0, 0])
    k = needed = 0
    for s in range(nseg):
        o, ln = int(seg_off[s]), int(seg_len[s])
        first, p, st, a0, a1 = k, 0, OK, 0, 0
        while p < ln and k < cap:
            left = ln - p
            if left < 4:
                st = INCOMPLETE_HEADER
                break
            h = _BE.unpack_from(slab, o + p)[0]
            if not h >> 31:
                st = FRAGMENTED
                break
            want = (h & 0x7FFFFFFF) + 4
            if left < want:
                st, a0, a1 = INCOMPLETE_MESSAGE, left & 0xFFFFFFFF, want & 0xFFFFFFFF
                break
            start.append(o + p)
            length.append(want)
            seg.append(s)
            k += 1
            p += want
        rows.append((first, k - first, p, st, a0, a1))
        needed += len(FM.true_starts(slab[o:o + ln])[0])
    return Framed(start, length, seg, rows, [k, needed, sum(1 for r in rows if r[3] != OK)])


def frame_streams_oracle(slab, seg_off, seg_len, max_records=None):
    """The same from the oracle: oracle_ffi.frame_stream on each segment's
    bytes with the capacity that is left, as a caller's per-connection loop
    would run it."""
    import oracle_ffi
    slab = bytes(slab)
    nseg = len(seg_off)
    cap = 1 << 62 if max_records is None else int(max_records)
    start, length, seg, rows = [], [], [], []
    if nseg == 0 or cap == 0:
        return Framed(start, length, seg, np.zeros((nseg, 6), np.uint64), [0, 0, 0])
    k = needed = 0
    for s in range(nseg):
        o, ln = int(seg_off[s]), int(seg_len[s])
        buf = slab[o:o + ln]
        room = min(cap - k, ln // 4 + 1)
        off, n, consumed, st, a0, a1 = oracle_ffi.frame_stream(buf, room)
        if k == cap:                                   # the caller's loop never looked at this segment
            assert (n, consumed, st) == (0, 0, OK)
        for i in range(n):
            start.append(o + int(off[i]))
            length.append(int(off[i + 1]) - int(off[i]))
            seg.append(s)
        rows.append((k, n, consumed, st, a0, a1))
        k += n
        needed += oracle_ffi.frame_stream(buf)[1]
    return Framed(start, length, seg, rows, [k, needed, sum(1 for r in rows if r[3] != OK)])


# ---------------------------------------------------------------------------
# slabs
# ---------------------------------------------------------------------------
class Slab:
    """Segments laid into one buffer with GAP bytes between them."""

    def __init__(self, front=0):
        self.parts = [GAP * ((front + 3) // 4)]
        self.parts[0] = self.parts[0][:front]
        self.pos = front
        self.off, self.len = [], []

    def add(self, data, gap=8, listed=True):
        data = bytes(data)
        if listed:
            self.off.append(self.pos)
            self.len.append(len(data))
        g = (GAP * (gap // 4 + 1))[:gap]
        self.parts += [data, g]
        self.pos += len(data) + gap
        return len(self.off) - 1

    def done(self):
        return b"".join(self.parts) + GAP * 4, np.array(self.off, np.uint64), np.array(self.len, np.uint64)


def _small_record(rng, xid):
    k = int(rng.integers(0, 4))
    if k == 0:
        return FM.reply28(xid & 0x7F7F)
    if k == 1:
        return FM.call(xid & 0x7F7F, rng.bytes(int(rng.integers(0, 40))))
    if k == 2:
        return FM.opaque(rng.bytes(int(rng.integers(0, 24))))
    return FM.reply(xid & 0x7F7F, rng.bytes(int(rng.integers(1, 60))))


@functools.lru_cache(maxsize=None)
def small_segments(nseg, seed=5):
    """nseg segments of 0-3 small records each, at odd offsets (gaps of 0-19
    GAP bytes)."""
    rng = np.random.default_rng(seed + nseg)
    sl = Slab(front=int(rng.integers(0, 16)))
    for s in range(nseg):
        n = int(rng.integers(0, 4))
        sl.add(b"".join(_small_record(rng, 64 * s + i) for i in range(n)), gap=int(rng.integers(0, 20)))
    return sl.done()


@functools.lru_cache(maxsize=None)
def reply_segments(nseg=66_000, seed=6):
    """nseg segments of 0-2 28-byte replies, back to back in 64-byte slots."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 3, nseg)
    slot = np.frombuffer(FM.reply28(0x1234) * 2 + GAP * 2, np.uint8)
    slab = np.tile(slot, nseg).tobytes() + GAP * 4
    return slab, np.arange(nseg, dtype=np.uint64) * np.uint64(64), (n * 28).astype(np.uint64)


def healthy(rng, xid):
    return FM.reply28(xid) + FM.call(xid + 1, rng.bytes(13)) + FM.opaque(rng.bytes(5))


# name -> (segment bytes, expected row tail (n, consumed, status, aux0, aux1))
def stop_cases():
    r2 = FM.reply28(7) + FM.reply(8, b"\x01" * 9)
    frag = bytes([0x00]) + FM.reply28(9)[1:]
    return {
        "empty": (b"", (0, 0, OK, 0, 0)),
        "one byte": (b"\x80", (0, 0, INCOMPLETE_HEADER, 0, 0)),
        "two bytes": (b"\x80\x00", (0, 0, INCOMPLETE_HEADER, 0, 0)),
        "three bytes": (b"\x80\x00\x00", (0, 0, INCOMPLETE_HEADER, 0, 0)),
        "cut by one": (r2 + FM.reply28(10)[:-1], (2, len(r2), INCOMPLETE_MESSAGE, 27, 28)),
        "fragmented first": (frag + FM.reply28(11), (0, 0, FRAGMENTED, 0, 0)),
        "fragmented third": (r2 + frag, (2, len(r2), FRAGMENTED, 0, 0)),
        "all ones": (b"\xff\xff\xff\xff" + b"\x00" * 4, (0, 0, INCOMPLETE_MESSAGE, 8, 0x80000003)),
    }


@functools.lru_cache(maxsize=None)
def stops_slab(seed=8):
    """Every stop case between two healthy segments. -> (slab, off, len,
    {name: segment index})."""
    rng = np.random.default_rng(seed)
    sl = Slab(front=3)
    where = {}
    sl.add(healthy(rng, 1), gap=5)
    for i, (name, (data, _)) in enumerate(stop_cases().items()):
        where[name] = sl.add(data, gap=4 + i % 3)
        sl.add(healthy(rng, 100 + 2 * i), gap=1 + i % 5)
    return sl.done() + (where,)


MARK_COUNTS = (KEEP - 1, KEEP, KEEP + 1, 2 * KEEP, 2 * KEEP + 1, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def marks_slab():
    """Segments of bare marks (80 00 00 00: empty records) around the count the
    chase keeps and around 64, a healthy segment between each."""
    rng = np.random.default_rng(9)
    sl = Slab(front=1)
    for i, n in enumerate(MARK_COUNTS):
        sl.add(b"\x80\x00\x00\x00" * n, gap=4)
        sl.add(healthy(rng, 10 * i), gap=3)
    return sl.done()


@functools.lru_cache(maxsize=None)
def long_slab():
    """One 1 MiB segment of 28..300-byte records (a single lane's chain), cut
    in its last record, between two small segments."""
    rng = np.random.default_rng(10)
    sl = Slab(front=7)
    sl.add(healthy(rng, 1))
    sl.add(FM.big_filler_stream(1 << 20)[:1 << 20], gap=9)
    sl.add(healthy(rng, 3))
    return sl.done()


@functools.lru_cache(maxsize=None)
def aligned_slab():
    """16 segments, one at each byte alignment of a 16-byte granule."""
    rng = np.random.default_rng(11)
    sl = Slab(front=0)
    for a in range(16):
        pad = (a - sl.pos) % 16
        sl.parts.append((GAP * 5)[:pad])
        sl.pos += pad
        sl.add(healthy(rng, 16 * a) + FM.reply28(a), gap=4)
    return sl.done()


@functools.lru_cache(maxsize=None)
def capacity_slab():
    """40 segments: small ones, segment 17 with 65 records, segment 30 with
    100, some stopped. -> (slab, off, len)."""
    rng = np.random.default_rng(12)
    sl = Slab(front=2)
    stops = list(stop_cases().values())
    for s in range(40):
        if s == 17:
            data = b"".join(FM.reply28(i) for i in range(65))
        elif s == 30:
            data = b"".join(FM.opaque(rng.bytes(i % 7)) for i in range(100))
        elif s % 9 == 4:
            data = stops[(s // 9) * 2 + 4][0] if (s // 9) * 2 + 4 < len(stops) else stops[1][0]
        else:
            data = b"".join(_small_record(rng, 64 * s + i) for i in range(int(rng.integers(0, 5))))
        sl.add(data, gap=int(rng.integers(0, 9)))
    return sl.done()


SLOT = 4096


@functools.lru_cache(maxsize=None)
def connection_slab(nconn=100, seed=13):
    """A slab of nconn connection slots of SLOT bytes, each filled to a random
    level with the oracle's encoding of mixed messages and (mostly) cut in its
    last record; slot 37 starts with a fragmented mark after two records, slot
    61 is empty. The rest of each slot holds stale bytes of other records.
    -> (slab, off, len)."""
    wire = FM.mixed_stream(3000, 47, 0, 200)
    starts, stop, st = FM.true_starts(wire)[:3]
    assert st == OK and stop == len(wire)
    starts = [int(x) for x in starts] + [len(wire)]
    rng = np.random.default_rng(seed)
    slab = bytearray((wire * (nconn * SLOT // len(wire) + 2))[5:5 + nconn * SLOT])   # stale bytes everywhere
    off = np.arange(nconn, dtype=np.uint64) * np.uint64(SLOT)
    ln = np.zeros(nconn, np.uint64)
    r = 0
    for c in range(nconn):
        if c == 61:
            continue
        fill = SLOT if c == 37 else int(rng.integers(200, SLOT + 1))
        first = r
        while starts[r + 1] - starts[first] <= fill:   # records [first, r) fit whole
            r += 1
        data = bytearray(wire[starts[first]:starts[r]])
        if c % 4 != 0:                                 # three of four slots end inside record r
            data += wire[starts[r]:starts[r] + min(fill - len(data), starts[r + 1] - starts[r] - 1)]
        if c == 37:
            assert r - first >= 3
            data[starts[first + 2] - starts[first]] &= 0x7F
        slab[c * SLOT:c * SLOT + len(data)] = data
        ln[c] = len(data)
        if r + 100 >= len(starts):
            r = 0
    return bytes(slab) + b"\0" * 16, off, ln
