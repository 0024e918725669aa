"""Host model of onc_fragment (records cut into fragments on the send side,
RFC 5531 §11) and the builders of the streams its tests use
(tests/test_fragment_encode_model.py and tests/test_fragment_host.py on the
CPU, tests/test_gpu_fragment_encode.py on the GPU).

Not a test file and not product code: plain numpy / Python restating the loop
written down in include/onc_rpc.h above onc_fragment. Expected bytes come
from here, from fragment_model.refragment (an independent statement of the
same cut) and from the oracle's encoder, never from the code under test.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

import fragment_model as M
import frame_model as FM

OK, ENC_BAD_DESCRIPTOR, ENC_WRITE_ZERO = 0, 104, 105
LAST = 0x80000000
MAX_FRAG_LIMIT = 0x7FFFFFFF
_BE = struct.Struct(">I")

TILE = 8192          # fragment.hip kFgTile: output bytes per wave and step
STAGE = 128          # fragment.hip kFgStage: records of a tile kept in LDS

GOLDEN_MAX_FRAGS = (1, 3, 4, 12, 16, 28, 100, MAX_FRAG_LIMIT)


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
def fragment(wire, rec_off, max_frag, out_cap=None):
    """onc_fragment of the records wire[rec_off[i]:rec_off[i+1]] ->
    dict(records: per record its fragments' bytes (None: nothing written),
    out_off uint64[n + 1], status int32[n], result uint64[3]); out_cap None:
    everything fits."""
    assert 1 <= max_frag <= MAX_FRAG_LIMIT
    wire = bytes(wire)
    ro = [int(x) for x in rec_off]
    n = len(ro) - 1
    pos = nf = multi = 0
    out_off, status, records = [], [], []
    for i in range(n):
        out_off.append(pos)
        L = ro[i + 1] - ro[i]
        if L == 0:
            status.append(OK)
            records.append(None)
            continue
        if L < 4:
            status.append(ENC_BAD_DESCRIPTOR)
            records.append(None)
            continue
        B = L - 4
        k = max(1, -(-B // max_frag))
        ln = 4 * k + B
        fits = out_cap is None or (pos <= out_cap and ln <= out_cap - pos)
        status.append(OK if fits else ENC_WRITE_ZERO)
        if fits:
            body = wire[ro[i] + 4:ro[i + 1]]
            parts = []
            for j in range(k - 1):
                parts.append(_BE.pack(max_frag) + body[j * max_frag:(j + 1) * max_frag])
            parts.append(_BE.pack(LAST | (B - (k - 1) * max_frag)) + body[(k - 1) * max_frag:])
            rec = b"".join(parts)
            assert len(rec) == ln
            records.append(rec)
        else:
            records.append(None)
        pos += ln
        nf += k
        multi += k > 1
    out_off.append(pos)
    return {"records": records, "out_off": np.array(out_off, np.uint64), "status": np.array(status, np.int32),
            "result": np.array([nf, pos, multi], np.uint64)}


def expected_out(model, size, sentinel):
    """The `size` bytes from `out` on after the call: OK records' fragments
    at their offsets, the sentinel everywhere else."""
    a = np.full(size, sentinel, np.uint8)
    for rec, off in zip(model["records"], model["out_off"]):
        if rec is not None:
            a[int(off):int(off) + len(rec)] = np.frombuffer(rec, np.uint8)
    return a


def stream_bytes(model):
    """The output as one stream (every record fits)."""
    return b"".join(r for r in model["records"] if r is not None)


def offsets_of(records, base=0):
    return np.concatenate(([base], base + np.cumsum([len(r) for r in records]))).astype(np.uint64)


def packed(records, base=0):
    """(wire, rec_off) of records back to back, `base` unused bytes in front."""
    return b"\xEE" * base + b"".join(records), offsets_of(records, base)


# ---------------------------------------------------------------------------
# what the copy does with a stream: positions, tiles, the 16-byte path
# ---------------------------------------------------------------------------
def mark_positions(model, max_frag):
    """Output positions of every mark, and which of them are synthesised
    continuation marks (not a record's first)."""
    pos, cont = [], []
    for rec, off in zip(model["records"], model["out_off"]):
        if rec is None:
            continue
        for j in range(max(1, -(-(len(rec) - 4) // (max_frag + 4)))):
            pos.append(int(off) + j * (max_frag + 4))
            cont.append(j > 0)
    return np.array(pos, np.int64), np.array(cont, bool)


def records_reaching_into_tiles(model, origin=0):
    """Per output tile, how many records that take bytes reach into it (`out`
    at `origin` bytes past a 16-byte aligned address)."""
    off = model["out_off"].astype(np.int64) + origin
    lo, hi = off[:-1], off[1:]
    keep = hi > lo
    lo, hi = lo[keep], hi[keep]
    ntiles = int((off[-1] + TILE - 1) // TILE)
    cnt = np.zeros(max(ntiles, 1), np.int64)
    for a, b in zip(lo // TILE, (hi - 1) // TILE):
        cnt[a:b + 1] += 1
    return cnt


def fast_path_pairs(wire_off, max_frag, shifts=range(16)):
    """{(source address mod 16, destination mod 16)} over the 16-byte output
    chunks that lie inside one fragment's body — those the copy moves with
    one unaligned 16-byte load and one aligned store — with the wire at a
    16-byte aligned address and `out` at `shift` past one, for every shift.
    The destination is the chunk's position in `out` (its address is
    aligned: position + shift = 0 mod 16), so a pair says which source
    alignment met which placement of `out`."""
    ro = [int(x) for x in wire_off]
    pairs = set()
    stride = max_frag + 4
    for shift in shifts:
        pos = 0
        for i in range(len(ro) - 1):
            L = ro[i + 1] - ro[i]
            if L < 4:
                continue
            B = L - 4
            k = max(1, -(-B // max_frag))
            for j in range(k):
                flen = min(max_frag, B - j * max_frag)
                b0 = pos + j * stride + 4                 # the fragment's body in out
                c = b0 + (-(b0 + shift)) % 16             # first aligned chunk at or after it
                if c + 16 <= b0 + flen:                   # (every later chunk of the body has the same pair)
                    src = ro[i] + 4 + j * max_frag + (c - b0)
                    pairs.add((src % 16, c % 16))
            pos += 4 * k + B
    return pairs


# ---------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------
ALIGN_MAX_FRAGS = (16, 17, 33, 100)
ALIGN_BODIES = (0, 1, 3, 15, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def alignment_stream(seed=41, reps=4):
    """Records with bodies of ALIGN_BODIES bytes in shuffled order, and
    between them records of at least 16 * 17 body bytes. In a packed stream
    the output runs ahead of the wire by four bytes per added mark, so a
    chunk's source and destination would differ by a multiple of 4 only:
    each round also holds an extent of 1, 2 or 3 bytes (no record: it takes
    wire bytes and no output), which moves every later source by that much."""
    rng = np.random.default_rng(seed)
    parts = []
    for r in range(reps):
        bodies = list(ALIGN_BODIES)
        rng.shuffle(bodies)
        for b in bodies:
            parts.append(FM.opaque(rng.bytes(b)))
        parts.append(FM.opaque(rng.bytes(16 * 17 + 1 + 2 * r)))
        parts.append(b"\x80" * (1 + r % 3))
    return packed(parts)


COUNT_EDGE_FS = (1, 4, 15, 16, 17)


@functools.lru_cache(maxsize=None)
def count_edges_stream(F, seed=43):
    """Bodies of 0, F-1, F, F+1, 2F, 2F+1 bytes, twice, shuffled."""
    rng = np.random.default_rng(seed + F)
    bodies = [0, F - 1, F, F + 1, 2 * F, 2 * F + 1] * 2
    rng.shuffle(bodies)
    return packed([FM.opaque(rng.bytes(b)) for b in bodies])


@functools.lru_cache(maxsize=None)
def empty_records_stream(n=3000, seed=47):
    """`n` bare marks (4-byte records: 2048 of them start in one 8 KiB tile,
    more than the staged window) between two ordinary records."""
    rng = np.random.default_rng(seed)
    return packed([FM.reply(1, rng.bytes(50))] + [FM.opaque(b"")] * n + [FM.reply(2, rng.bytes(33))])


@functools.lru_cache(maxsize=None)
def short_records_stream(n=500, size=24, seed=53):
    rng = np.random.default_rng(seed)
    return packed([FM.opaque(rng.bytes(size - 4)) for _ in range(n)])


@functools.lru_cache(maxsize=None)
def large_record_stream(body=100_000, seed=59):
    rng = np.random.default_rng(seed)
    return packed([FM.reply28(1), FM.opaque(rng.bytes(body)), FM.reply28(2)])


TILE_MARK_FRAG = 1000


@functools.lru_cache(maxsize=None)
def tile_mark_stream(d, origin, seed=61):
    """At max_frag = TILE_MARK_FRAG a synthesised (continuation) mark starts
    `d` bytes before tile 1's first byte (`out` at `origin` bytes past a
    16-byte aligned address: that byte is out[TILE - origin])."""
    rng = np.random.default_rng(seed)
    F = TILE_MARK_FRAG
    j = (TILE - 100) // (F + 4)                     # the mark of fragment j of the second record
    lead = TILE - origin - d - j * (F + 4) - 4      # body of the first record: one fragment
    assert 0 <= lead <= F
    return packed([FM.opaque(rng.bytes(lead)), FM.opaque(rng.bytes(j * F + 3000)), FM.reply28(3)])


@functools.lru_cache(maxsize=None)
def tile_record_boundary_stream(origin, seed=67):
    """A record starts exactly at tile 1's first byte at max_frag =
    TILE_MARK_FRAG (the records before it fill tile 0 to the last byte)."""
    rng = np.random.default_rng(seed)
    F = TILE_MARK_FRAG
    # first record: 5 full fragments and a rest; then small records up to the boundary
    first = FM.opaque(rng.bytes(5 * F + 77))
    used = 6 * 4 + 5 * F + 77
    left = TILE - origin - used
    recs = [first]
    while left > 300:
        recs.append(FM.opaque(rng.bytes(96)))
        left -= 100
    recs.append(FM.opaque(rng.bytes(left - 4)))
    return packed(recs + [FM.opaque(rng.bytes(2500)), FM.reply28(4)])


TILE_RUN_FRAG = 1000


def _run_body(ln, F=TILE_RUN_FRAG):
    """The body length of a record whose fragments take `ln` output bytes at
    max_frag F (None: no record does)."""
    if ln < 4:
        return None
    k = -(-ln // (F + 4))
    B = ln - 4 * k
    return B if B >= 0 and max(1, -(-B // F)) == k else None


def tile_run_units():
    """tile_walk_model.Units of frag_copy at max_frag TILE_RUN_FRAG: an entry
    is a record's fragments (a short one: a bare mark) or, of no output, an
    extent of 0..3 bytes that is no record. So positions repeat here too: the
    plan gives such an extent the next record's position."""
    import tile_walk_model as TW
    return TW.Units(TILE, (200, 600), 4, lambda ln: ln == 0 or _run_body(ln) is not None)


@functools.lru_cache(maxsize=None)
def tile_run_stream(kind, ntiles, origin, seed=79):
    """-> (wire, rec_off): tile_walk_model.layout(kind, ntiles, origin) as
    records for max_frag TILE_RUN_FRAG. The positions of the walk are the
    model's out_off."""
    import tile_walk_model as TW
    entries, _ = TW.layout(kind, ntiles, origin, tile_run_units())
    rng = np.random.default_rng(seed + ntiles)
    parts = []
    for i, (ln, _) in enumerate(entries):
        parts.append(bytes([0x80]) * (i % 4) if ln == 0 else FM.opaque(rng.bytes(_run_body(ln))))
    return packed(parts)


def non_record_extents(kind, seed=71):
    """(wire, rec_off): extents of 0, 1, 2 and 3 bytes — no records — first,
    last, adjacent and between records ('mixed'), or nothing else ('only')."""
    rng = np.random.default_rng(seed)
    r = lambda b: FM.opaque(rng.bytes(b))
    junk = lambda k: bytes([0x80]) * k              # would read as a mark's first bytes if it were read
    if kind == "mixed":
        parts = [b"", junk(1), r(20), junk(3), junk(2), b"", r(0), junk(1), r(40), b"", junk(2), r(7), junk(3), b""]
    elif kind == "only":
        parts = [junk(1), b"", junk(3), junk(2), b"", b""]
    else:
        raise KeyError(kind)
    return packed(parts)


def short_records(n, seed=73):
    """n records of 4..40 bytes (the plan's blocks are 256 records)."""
    rng = np.random.default_rng(seed + n)
    return packed([FM.opaque(rng.bytes(int(b))) for b in rng.integers(0, 37, n)])
