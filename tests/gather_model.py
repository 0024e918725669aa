"""Host model of onc_piece_offsets / onc_gather_pieces (a piece list written
as one stream on the device) and the builders of the piece lists their tests
use (tests/test_gather_model.py on the CPU, tests/test_gpu_gather.py on the
GPU).

Not a test file and not product code: plain numpy / Python restating the two
loops written down in include/onc_rpc.h above onc_piece_offsets. Expected
positions, results and bytes come from here, from fragment_iov_model.gather
and from fragment_encode_model.fragment of the packed stream, never from the
code under test.
"""
from __future__ import annotations

import functools

import numpy as np

from fragment_iov_model import PIECE_DTYPE, PIECE_HDR, PIECE_MARK, PIECE_PAYLOAD

TILE = 8192          # gather.hip kGaTile: bytes of `out` per wave and step
STAGE = 128          # gather.hip kGaStage: pieces of a tile kept in LDS
U64 = (1 << 64) - 1


def make_pieces(items):
    """[(off, len, src), ...] -> PIECE_DTYPE array."""
    return np.array(list(items), PIECE_DTYPE) if len(items) else np.zeros(0, PIECE_DTYPE)


def source_lens(sources):
    return [0 if s is None else len(s) for s in sources]


# ---------------------------------------------------------------------------
# the two loops
# ---------------------------------------------------------------------------
def ok(off, ln, src, lens):
    """The piece lies inside its source (Python integers: nothing wraps)."""
    return ln == 0 or (src <= 2 and off <= lens[src] and ln <= lens[src] - off)


def piece_offsets(pieces, lens):
    """-> (piece_pos uint64[n + 1], result uint64[3] = {stream bytes, bad
    pieces, first bad piece (n: none)})."""
    n = len(pieces)
    pos = bad = 0
    first_bad = n
    piece_pos = []
    for i, (off, ln, src) in enumerate(pieces.tolist()):
        piece_pos.append(pos)
        if not ok(off, ln, src, lens):
            bad += 1
            first_bad = min(first_bad, i)
        pos += ln
    piece_pos.append(pos)
    return np.array(piece_pos, np.uint64), np.array([pos, bad, first_bad], np.uint64)


def gather(pieces, piece_pos, sources, start, count, out, lens=None):
    """Stream bytes [start, start + count) into out[0, count) (a uint8 array,
    changed in place: what the loop does not write stays). `sources`: three
    uint8 arrays or None; `lens`: the lengths handed to the call (default: the
    arrays')."""
    lens = source_lens(sources) if lens is None else lens
    end = min(start + count, U64)
    for i, (off, ln, src) in enumerate(pieces.tolist()):
        p = int(piece_pos[i])
        a, b = max(p, start), min(p + ln, end)
        if a < b and ok(off, ln, src, lens):
            out[a - start:b - start] = sources[src][off + (a - p):off + (b - p)]
    return out


def stream(pieces, sources, lens=None, fill=0):
    """The whole stream (bad pieces' bytes = `fill`)."""
    lens = source_lens(sources) if lens is None else lens
    pos, res = piece_offsets(pieces, lens)
    out = np.full(int(res[0]), fill, np.uint8)
    return gather(pieces, pos, sources, 0, int(res[0]), out, lens)


# ---------------------------------------------------------------------------
# what a list looks like to the copy kernel (out 16-byte aligned, window from 0)
# ---------------------------------------------------------------------------
def pieces_reaching_into_tiles(pieces):
    """Per 8 KiB tile of the stream, how many pieces stand in it: the ones
    with a byte in it and the empty ones that start in it."""
    ln = pieces["len"].astype(np.int64)
    pos = np.concatenate(([0], np.cumsum(ln)))
    cnt = np.zeros(int(pos[-1] // TILE) + 1, np.int64)
    for p, l in zip(pos[:-1].tolist(), ln.tolist()):
        cnt[p // TILE:(p + max(l, 1) - 1) // TILE + 1] += 1
    return cnt


def zero_runs(pieces):
    """[(stream position, run length)] of the maximal runs of empty pieces."""
    ln = pieces["len"].astype(np.int64)
    pos = np.concatenate(([0], np.cumsum(ln)))
    runs, i = [], 0
    while i < len(ln):
        if ln[i] == 0:
            j = i
            while j < len(ln) and ln[j] == 0:
                j += 1
            runs.append((int(pos[i]), j - i))
            i = j
        else:
            i += 1
    return runs


def alignment_pairs(pieces, min_len=31):
    """{(source offset % 16, stream position % 16)} of the pieces long enough
    to hold a whole aligned 16-byte chunk of the output."""
    ln = pieces["len"].astype(np.int64)
    pos = np.concatenate(([0], np.cumsum(ln)))[:-1]
    keep = ln >= min_len
    return set(zip((pieces["off"][keep] % 16).tolist(), (pos[keep] % 16).tolist()))


# ---------------------------------------------------------------------------
# piece lists: (pieces, [marks, hdr, payload]). Sources are random bytes.
# ---------------------------------------------------------------------------
def _sources(seed, n0, n1, n2):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8) if n else None for n in (n0, n1, n2)]


@functools.lru_cache(maxsize=None)
def one_byte_pieces(n=20_000):
    """n pieces of one byte each, from all three sources: 8192 of them in
    every tile."""
    src = _sources(1, 997, 1499, 4001)
    rng = np.random.default_rng(2)
    s = rng.integers(0, 3, n)
    lens = np.array(source_lens(src))
    off = rng.integers(0, 1 << 30, n) % lens[s]
    return make_pieces(list(zip(off.tolist(), [1] * n, s.tolist()))), src


@functools.lru_cache(maxsize=None)
def zero_run_list(run):
    """A run of `run` empty pieces inside tile 0 (at stream position 3000) and
    another exactly on the boundary of tiles 1 and 2 (position 16384), between
    pieces of 1..600 bytes; the empty ones point anywhere, past the sources'
    ends included. The unused source is NULL with length 0."""
    src = _sources(10 + run, 0, 700, 5000)
    rng = np.random.default_rng(20 + run)
    items, pos = [], 0

    def fill_to(target):
        nonlocal pos
        while pos < target:
            s = int(rng.integers(1, 3))
            ln = min(int(rng.integers(1, 601)), target - pos)
            items.append((int(rng.integers(0, len(src[s]) - ln + 1)), ln, s))
            pos += ln

    def empties(k):
        for i in range(k):
            items.append(((U64, 0, 1 << 40, 123)[i % 4], 0, (0, 1, 2, 7)[i % 4]))

    fill_to(3000)
    empties(run)
    fill_to(2 * TILE)
    empties(run)
    fill_to(2 * TILE + 3000)
    empties(1)
    return make_pieces(items), src


@functools.lru_cache(maxsize=None)
def tile_run_list(kind, ntiles, origin, seed=90):
    """-> (pieces, sources): tile_walk_model.layout(kind, ntiles, origin) as
    pieces from the header and payload sources (the marks source is NULL); the
    empty ones point anywhere. For a window from 0 into `out` at `origin` past
    an aligned address the positions of the walk are piece_pos."""
    import tile_walk_model as TW
    entries, _ = TW.layout(kind, ntiles, origin)
    longest = max(ln for ln, _ in entries)
    src = _sources(seed + ntiles, 0, 700, max(5000, longest + 77))
    rng = np.random.default_rng(seed + 1 + ntiles)
    items = []
    for i, (ln, _) in enumerate(entries):
        if ln == 0:
            items.append(((U64, 0, 1 << 40, 123)[i % 4], 0, (0, 1, 2, 7)[i % 4]))
        else:
            s = PIECE_HDR if ln <= 600 and i % 2 else PIECE_PAYLOAD
            items.append((int(rng.integers(0, len(src[s]) - ln + 1)), ln, s))
    return make_pieces(items), src


@functools.lru_cache(maxsize=None)
def long_piece_list(length=100_000):
    """One piece of `length` bytes (more than 12 tiles) between small ones; the
    piece after it starts on the last byte of a tile."""
    src = _sources(30, 64, 300, length + 77)
    items = [(0, 4, PIECE_MARK), (10, 33, PIECE_HDR), (50, length, PIECE_PAYLOAD), (4, 4, PIECE_MARK)]
    pos = 4 + 33 + length + 4
    pad = (-pos - 1) % TILE                          # the next piece starts at TILE * k - 1
    items.append((7, pad, PIECE_PAYLOAD))
    items += [(100, 50, PIECE_HDR), (8, 4, PIECE_MARK), (3, 29, PIECE_PAYLOAD)]
    return make_pieces(items), src


@functools.lru_cache(maxsize=None)
def alignment_grid(length=40):
    """For every (source offset % 16, stream position % 16) a piece of
    `length` bytes (a whole aligned output chunk lies inside it), from the
    payload and, every other one, the header source; pieces of 1..16 mark bytes
    in between move the stream position."""
    src = _sources(40, 64, 4096, 4096)
    items, pos, k = [], 0, 0
    for sa in range(16):
        for oa in range(16):
            pad = (oa - pos) % 16
            if pad:
                items.append((k % 40, pad, PIECE_MARK))
                pos += pad
            s = PIECE_PAYLOAD if k % 2 else PIECE_HDR
            items.append((16 * (k % 200) + sa, length, s))
            pos += length
            k += 1
    return make_pieces(items), src


@functools.lru_cache(maxsize=None)
def repeated_list(times=5000):
    """The same 7 source bytes `times` times over."""
    src = _sources(50, 0, 0, 64)
    return make_pieces([(13, 7, PIECE_PAYLOAD)] * times), [None, None, src[2]]


@functools.lru_cache(maxsize=None)
def descending_list(n=900):
    """Pieces in descending source order, overlapping their neighbours."""
    src = _sources(60, 16, 5000, 30000)
    rng = np.random.default_rng(61)
    items = []
    for i in range(n):
        s = PIECE_PAYLOAD if i % 3 else PIECE_HDR
        ln = int(rng.integers(1, 90))
        top = len(src[s]) - 90
        items.append((top - top * i // n, ln, s))
    items.insert(n // 2, (0, 16, PIECE_MARK))
    return make_pieces(items), src


BAD_SRC_LENS = (48, 301, 1)        # marks, hdr, payload: the payload source is ONE byte long


@functools.lru_cache(maxsize=None)
def bad_piece_list(where):
    """Bad pieces `where` = 'first', 'last' or 'mid' (in the middle of tile 0,
    and again across the boundary of tiles 0 and 1) among good ones:
      src = 3; off = len[src] + 1 with len = 1 (the one-byte payload source);
      off + len one past the source; off = 2^64 - 1 with len = 2;
    and a zero-length piece at an impossible offset, which is OK. Every bad
    piece points past its source's end only."""
    src = _sources(70, *BAD_SRC_LENS)
    L = BAD_SRC_LENS
    bad = [(5, 9, 3), (L[2] + 1, 1, PIECE_PAYLOAD), (L[1] - 10, 11, PIECE_HDR), (U64, 2, PIECE_MARK),
           (L[1] + 1, 40, PIECE_HDR)]
    fine = (U64, 0, PIECE_HDR)                        # empty: OK wherever it points
    rng = np.random.default_rng(71)

    def good(nbytes):
        out = []
        while nbytes > 0:
            if rng.integers(0, 5) == 0:
                out.append((0, 1, PIECE_PAYLOAD))     # the whole one-byte source
                nbytes -= 1
                continue
            ln = min(int(rng.integers(1, 200)), nbytes)
            out.append((int(rng.integers(0, L[1] - ln + 1)), ln, PIECE_HDR))
            nbytes -= ln
        return out

    if where == "first":
        items = bad + [fine] + good(9000)
    elif where == "last":
        items = good(9000) + [fine] + bad
    else:
        items = good(4000) + bad[:2] + [fine] + good(TILE - 4000 - 10 - 30) + bad[2:] + good(3000)
    return make_pieces(items), src
