"""Host model of onc_fragment_iov (the vectored encode's records cut into
fragments without a byte copied) and the builders of the entry lists its
tests use (tests/test_fragment_iov_model.py and tests/test_fragment_iov_host.py
on the CPU, tests/test_gpu_fragment_iov.py on the GPU).

Not a test file and not product code: plain numpy / Python restating the loop
written down in include/onc_rpc.h above onc_fragment_iov. Expected pieces,
marks and tables come from here, expected bytes from
fragment_encode_model.fragment of the packed stream and from the oracle's
encoder, never from the code under test.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

OK, ENC_BAD_DESCRIPTOR, ENC_WRITE_ZERO = 0, 104, 105
LAST = 0x80000000
MAX_FRAG_LIMIT = 0x7FFFFFFF
PIECE_MARK, PIECE_HDR, PIECE_PAYLOAD = 0, 1, 2
_BE = struct.Struct(">I")

TILE = 512           # fragment_iov.hip kFvTile: pieces per wave and step
STAGE = 128          # fragment_iov.hip kFvStage: records of a tile kept in LDS

# include/onc_rpc.h onc_iov_rec and onc_frag_piece
IOV_DTYPE = np.dtype({"names": ["hdr_off", "payload_off", "wire_off", "hdr_len", "payload_len"],
                      "formats": ["<u8", "<u8", "<u8", "<u4", "<u4"], "offsets": [0, 8, 16, 24, 28], "itemsize": 32})
PIECE_DTYPE = np.dtype({"names": ["off", "len", "src"], "formats": ["<u8", "<u4", "<u4"], "offsets": [0, 8, 12],
                        "itemsize": 16})


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
def fragment_iov(iov, max_frag, rec_max_frag=None, max_pieces=None, marks_cap=None):
    """onc_fragment_iov of the entries -> dict(pieces PIECE_DTYPE[written],
    marks bytes (the written ones), out_off / piece_off uint64[n + 1], status
    int32[n], result uint64[4]); a capacity None: everything fits. What is
    written is a prefix of both arrays: nothing follows the first record that
    does not fit."""
    assert 1 <= max_frag <= MAX_FRAG_LIMIT
    n = len(iov)
    pos = nf = multi = np_ = 0
    out_off, piece_off, status, pieces, marks = [], [], [], [], []
    for i in range(n):
        out_off.append(pos)
        piece_off.append(np_)
        hl, pl = int(iov["hdr_len"][i]), int(iov["payload_len"][i])
        L = hl + pl
        F = max_frag if rec_max_frag is None else int(rec_max_frag[i])
        if L == 0:
            status.append(OK)
            continue
        if hl < 4 or F < 1 or F > MAX_FRAG_LIMIT:
            status.append(ENC_BAD_DESCRIPTOR)
            continue
        Hb, B = hl - 4, L - 4
        k = max(1, -(-B // F))
        x = 1 if (Hb % F != 0 and pl > 0) else 0
        e = 1 if B == 0 else 2 * k + x
        fits = ((max_pieces is None or (np_ <= max_pieces and e <= max_pieces - np_)) and
                (marks_cap is None or (4 * nf <= marks_cap and 4 * k <= marks_cap - 4 * nf)))
        status.append(OK if fits else ENC_WRITE_ZERO)
        if fits:
            assert len(pieces) == np_ and len(marks) == nf
            ho, po = int(iov["hdr_off"][i]), int(iov["payload_off"][i])
            for j in range(k):
                a, b = j * F, min((j + 1) * F, B)
                marks.append(_BE.pack((LAST if j == k - 1 else 0) | (b - a)))
                pieces.append((4 * (nf + j), 4, PIECE_MARK))
                if a < Hb and b > a:
                    pieces.append((ho + 4 + a, min(b, Hb) - a, PIECE_HDR))
                if b > Hb and pl > 0:
                    s = max(a, Hb)
                    pieces.append((po + s - Hb, b - s, PIECE_PAYLOAD))
            assert len(pieces) == np_ + e
        pos += 4 * k + B
        nf += k
        multi += k > 1
        np_ += e
    out_off.append(pos)
    piece_off.append(np_)
    return {"pieces": np.array(pieces, PIECE_DTYPE) if pieces else np.zeros(0, PIECE_DTYPE),
            "marks": b"".join(marks), "out_off": np.array(out_off, np.uint64),
            "piece_off": np.array(piece_off, np.uint64), "status": np.array(status, np.int32),
            "result": np.array([nf, pos, multi, np_], np.uint64)}


def gather(pieces, marks, hdr, payload):
    """The stream a writev() of the pieces sends: each piece's slice of its
    source, in order."""
    src = {PIECE_MARK: bytes(marks), PIECE_HDR: bytes(hdr), PIECE_PAYLOAD: bytes(payload)}
    out = []
    for off, ln, s in pieces.tolist():
        part = src[s][off:off + ln]
        assert len(part) == ln > 0, "a piece outside its source, or an empty one"
        out.append(part)
    return b"".join(out)


def records_reaching_into_tiles(model):
    """Per tile of the piece array, how many records that take pieces reach
    into it."""
    off = model["piece_off"].astype(np.int64)
    lo, hi = off[:-1], off[1:]
    keep = hi > lo
    cnt = np.zeros(max(int((off[-1] + TILE - 1) // TILE), 1), np.int64)
    for a, b in zip(lo[keep] // TILE, (hi[keep] - 1) // TILE):
        cnt[a:b + 1] += 1
    return cnt


# ---------------------------------------------------------------------------
# entry lists: (iov, hdr, payload, packed wire, rec_off). The header buffer
# and the payload arena hold what the entries point at, with unused bytes
# between the slices; the packed wire is the same records back to back.
# ---------------------------------------------------------------------------
def build(splits, seed=1):
    """Entries for (hdr_len, payload_len) pairs. A header of at least four
    bytes starts with the record's own single-fragment mark (never read)."""
    rng = np.random.default_rng(seed)
    iov = np.zeros(len(splits), IOV_DTYPE)
    hdr, pay, wire, off = [b"\xC3" * 5], [b"\x3C" * 3], [], [0]
    hpos, ppos = 5, 3
    for i, (hl, pl) in enumerate(splits):
        h = rng.bytes(hl)
        if hl >= 4:
            h = _BE.pack(LAST | ((hl + pl - 4) & 0x7FFFFFFF)) + h[4:]
        p = rng.bytes(pl)
        iov[i] = (hpos, ppos, 0xDEAD0000 + i, hl, pl)      # wire_off: ignored by the call
        hdr += [h, b"\xC3" * (i % 3)]
        pay += [p, b"\x3C" * (i % 5)]
        hpos += hl + i % 3
        ppos += pl + i % 5
        wire.append(h + p)
        off.append(off[-1] + hl + pl)
    return iov, b"".join(hdr), b"".join(pay), b"".join(wire), np.array(off, np.uint64)


def random_splits(n, seed, hmax=60, pmax=120):
    """Valid records (a header of 4..hmax bytes, a payload of 0..pmax) and,
    one in eight, an entry of no bytes."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        if rng.integers(0, 8) == 0:
            out.append((0, 0))
        else:
            out.append((int(rng.integers(4, hmax + 1)), int(rng.integers(0, pmax + 1)) * int(rng.integers(0, 4) > 0)))
    return out


BOUNDARY_FS = (1, 4, 15, 16, 17)


@functools.lru_cache(maxsize=None)
def boundary_stream(F):
    """Every header length of {1, 3, 4, 5, 4+F-1, 4+F, 4+F+1, 4+2F} with
    every payload length of {0, 1, F-1, F, F+1, 2F+1}, a payload without a
    header, and entries of no bytes first, last and adjacent."""
    hs = [1, 3, 4, 5, 4 + F - 1, 4 + F, 4 + F + 1, 4 + 2 * F]
    ps = [0, 1, F - 1, F, F + 1, 2 * F + 1]
    splits = [(0, 0)]
    for a, h in enumerate(hs):
        for b, p in enumerate(ps):
            splits.append((h, p))
            if (a + b) % 7 == 0:
                splits += [(0, 0), (0, 0)]
    splits += [(0, 9), (0, 0)]
    return build(splits, seed=100 + F)


STRADDLE_F = 7
STRADDLE_KINDS = {1: PIECE_HDR, 2: PIECE_MARK, 3: PIECE_HDR, 4: PIECE_PAYLOAD, 5: PIECE_MARK, 6: PIECE_PAYLOAD}


@functools.lru_cache(maxsize=None)
def tile_straddle_stream(t):
    """At max_frag STRADDLE_F the record (14, 10) is the seven pieces
    M H M H P M P (10 header bytes of the body: its second fragment holds 3 of
    them, then 4 payload bytes). Bare marks of one piece each before it put
    its piece t at tile 1's first place."""
    return build([(4, 0)] * (TILE - t) + [(14, 10)] + [(8, 3)] * 5, seed=200 + t)


TILE_RUN_F = 7


def _run_split(e, i, F=TILE_RUN_F):
    """(hdr_len, payload_len) of a record of exactly `e` pieces at max_frag F;
    e == 0: by turns an entry of no bytes and a header too short to be one
    (ENC_BAD_DESCRIPTOR), neither of which takes a piece."""
    if e == 0:
        return (0, 0) if i % 2 == 0 else (1 + i % 3, i % 5)
    if e == 1:
        return 4, 0                                  # a bare mark
    k = e // 2
    if e % 2 == 0:
        return 4 + k * F, 0                          # k fragments of header bytes: mark + piece each
    return 4 + 3, k * F - 3                          # the first fragment holds header and payload bytes


def tile_run_units():
    """tile_walk_model.Units of fragiov_fill: positions count pieces, a tile
    is TILE of them, and an entry is a record's pieces. Entries of no bytes
    and bad descriptors take none, so positions repeat here too: the plan
    gives them the next record's first piece."""
    import tile_walk_model as TW
    return TW.Units(TILE, (8, 30), 1)


@functools.lru_cache(maxsize=None)
def tile_run_stream(kind, ntiles):
    """tile_walk_model.layout(kind, ntiles, 0) in pieces, as entries for
    max_frag TILE_RUN_F. The positions of the walk are the model's piece_off."""
    import tile_walk_model as TW
    entries, _ = TW.layout(kind, ntiles, 0, tile_run_units())
    return build([_run_split(e, i) for i, (e, _) in enumerate(entries)], seed=800 + ntiles)


@functools.lru_cache(maxsize=None)
def bare_marks_stream(n=3000):
    """`n` bare-mark records of one piece each (512 of them start in one tile,
    more than the staged window), entries of no bytes between them, between
    two ordinary records."""
    splits = [(30, 50)]
    for i in range(n):
        splits.append((4, 0))
        if i % 2:
            splits.append((0, 0))
    return build(splits + [(20, 33)], seed=300)


@functools.lru_cache(maxsize=None)
def large_record_stream(payload=100_000):
    """One record of more pieces than several tiles hold (at max_frag 7:
    2 x 14290 + 1) between two small ones."""
    return build([(28, 0), (40, payload), (28, 5)], seed=400)


@functools.lru_cache(maxsize=None)
def short_records(n):
    """n records of 4..40 bytes (the plan's blocks are 256 records)."""
    rng = np.random.default_rng(500 + n)
    splits = []
    for L in rng.integers(4, 41, n):
        h = int(rng.integers(4, int(L) + 1))
        splits.append((h, int(L) - h))
    return build(splits, seed=600 + n)


PER_RECORD_LIMITS = (1, 3, 16, 100, MAX_FRAG_LIMIT, 0, 0x80000000, 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def per_record_stream(n=64):
    """Records with a limit each, the valid and the invalid values mixed so
    that every invalid entry has valid neighbours on both sides."""
    rng = np.random.default_rng(700)
    stream = build(random_splits(n, 701, hmax=40, pmax=90), seed=702)
    lim = np.array([PER_RECORD_LIMITS[(3 * i + i // 8) % len(PER_RECORD_LIMITS)] for i in range(n)], np.uint32)
    bad = np.nonzero((lim < 1) | (lim > MAX_FRAG_LIMIT))[0]
    for i in bad:                                    # (an invalid limit never follows another)
        if i + 1 < n and (lim[i + 1] < 1 or lim[i + 1] > MAX_FRAG_LIMIT):
            lim[i + 1] = int(rng.choice([1, 3, 16]))
    return stream, lim
