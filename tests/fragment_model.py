"""Host model of multi-fragment record streams (RFC 5531 §11) and the
builders of the streams the fragment tests use (tests/test_fragment_model.py
on the CPU, tests/test_gpu_fragments.py on the GPU).

Not a test file and not product code: plain numpy / Python restating the two
loops written down in include/onc_rpc.h — fragment framing
(onc_frame_fragments: the expected_message_len loop without the
last-fragment test) and reassembly (onc_defragment: per record one mark with
the last-fragment bit and the total length, then the fragments' bodies) —
plus builders that cut a stream of single-fragment records into fragments.
Expected bytes come from here and from the oracle's encoder, never from the
code under test.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

import frame_model as FM

OK, INCOMPLETE_MESSAGE, INCOMPLETE_HEADER, FRAGMENTED = 0, 1, 2, 3
ENC_TOO_LONG, ENC_WRITE_ZERO = 100, 105
LAST = 0x80000000
_BE = struct.Struct(">I")


# ---------------------------------------------------------------------------
# the two loops
# ---------------------------------------------------------------------------
def frame_fragments(buf, max_frags=None):
    """(frag_off uint64[n + 1], n, consumed, status, aux0, aux1)."""
    buf = bytes(buf)
    ln = len(buf)
    n_max = ln // 4 + 1 if max_frags is None else max_frags
    offs = []
    p, st, a0, a1 = 0, OK, 0, 0
    while p < ln and len(offs) < n_max:
        if ln - p < 4:
            st = INCOMPLETE_HEADER
            break
        want = (_BE.unpack_from(buf, p)[0] & 0x7FFFFFFF) + 4
        if ln - p < want:
            st, a0, a1 = INCOMPLETE_MESSAGE, ln - p, want & 0xFFFFFFFF
            break
        offs.append(p)
        p += want
    return np.array(offs + [p], np.uint64), len(offs), p, st, a0, a1


def defragment(buf, frag_off, out_cap=None):
    """onc_defragment of the fragments buf[frag_off[j]:frag_off[j+1]] ->
    dict(records: the reassembled bytes of every complete record, rec_off
    uint64[n + 1], status int32[n], result uint64[6]); status from out_cap
    (None: everything fits)."""
    buf = bytes(buf)
    frag_off = [int(x) for x in frag_off]
    nfrag = len(frag_off) - 1
    records, multi = [], 0
    bodies, first = [], 0
    for j in range(nfrag):
        lo, hi = frag_off[j], frag_off[j + 1]
        bodies.append(buf[lo + 4:hi])
        if buf[lo] & 0x80:
            body = b"".join(bodies)
            records.append(body)
            multi += len(bodies) > 1
            bodies, first = [], j + 1
    rec_off, status, out = [0], [], []
    for body in records:
        if len(body) >= 1 << 31:
            status.append(ENC_TOO_LONG)
            out.append(None)
            rec_off.append(rec_off[-1])
            continue
        rec = _BE.pack(LAST | len(body)) + body
        end = rec_off[-1] + len(rec)
        fits = out_cap is None or end <= out_cap
        status.append(OK if fits else ENC_WRITE_ZERO)
        out.append(rec if fits else None)
        rec_off.append(end)
    result = [len(records), frag_off[first], rec_off[-1], nfrag - first, sum(len(b) for b in bodies), multi]
    return {"records": out, "rec_off": np.array(rec_off, np.uint64), "status": np.array(status, np.int32),
            "result": np.array(result, np.uint64)}


def expected_out(model, size, sentinel):
    """The `size` bytes from `out` on after the call: OK records at their
    offsets, the sentinel everywhere else."""
    a = np.full(size, sentinel, np.uint8)
    for rec, off in zip(model["records"], model["rec_off"]):
        if rec is not None:
            a[int(off):int(off) + len(rec)] = np.frombuffer(rec, np.uint8)
    return a


# ---------------------------------------------------------------------------
# cutting records into fragments
# ---------------------------------------------------------------------------
def fragment(body, cuts):
    """One record body as len(cuts) + 1 fragments cut at the (sorted) body
    offsets `cuts`; equal cuts give zero-length fragments."""
    edges = [0] + sorted(int(c) for c in cuts) + [len(body)]
    parts = []
    for i in range(len(edges) - 1):
        piece = body[edges[i]:edges[i + 1]]
        last = LAST if i == len(edges) - 2 else 0
        parts.append(_BE.pack(last | len(piece)) + piece)
    return b"".join(parts)


def refragment(wire, rec_off, cuts_of):
    """A stream of single-fragment records (bytes + offsets) with record i
    cut at the body offsets cuts_of(i, body length)."""
    wire = bytes(wire)
    parts = []
    for i in range(len(rec_off) - 1):
        body = wire[int(rec_off[i]) + 4:int(rec_off[i + 1])]
        parts.append(fragment(body, cuts_of(i, len(body))))
    return b"".join(parts)


def random_cuts(seed, p_cut=0.6, max_cuts=6):
    """cuts_of for refragment: seeded random cut points, zero-length cuts
    (repeated points, cuts at 0 and at the end) included."""
    rng = np.random.default_rng(seed)

    def cuts_of(i, n):
        if rng.random() > p_cut:
            return []
        k = int(rng.integers(1, max_cuts + 1))
        cuts = rng.integers(0, n + 1, k).tolist()
        if rng.random() < 0.3:
            cuts.append(cuts[0])
        return cuts
    return cuts_of


def fixed_cuts(size):
    """cuts_of for refragment: every `size` body bytes, as a sender flushing
    a fixed buffer does."""
    return lambda i, n: list(range(size, n, size))


def golden_stream(golden):
    """(wire bytes, rec_off uint64[n + 1]): the golden vectors
    (tests/golden/vectors.json) whose mark says their own length with the
    last-fragment bit — those a stream can carry back to back; 40 of the 43
    (the other three test expected_message_len on marks that lie)."""
    recs = []
    for sect in ("messages", "errors", "xdrlib", "derived_errors"):
        for v in golden[sect]:
            r = bytes.fromhex(v["hex"])
            if len(r) >= 4 and _BE.unpack_from(r, 0)[0] == LAST | (len(r) - 4):
                recs.append(r)
    off = np.concatenate(([0], np.cumsum([len(r) for r in recs]))).astype(np.uint64)
    return b"".join(recs), off


def clear_last_bits(buf, frag_off, which):
    """buf with the last-fragment bit cleared on the marks frag_off[j], j in which."""
    b = bytearray(buf)
    for j in which:
        b[int(frag_off[j])] &= 0x7F
    return bytes(b)


# ---------------------------------------------------------------------------
# streams for the framer's fragment mode (frame_chunk = 64 unless said)
# ---------------------------------------------------------------------------
EDGE_CHUNK = 64


def _low(rng, n):
    return rng.integers(0, 128, n, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def continuation_stream(span_chunks, chunk=EDGE_CHUNK, rounds=5, seed=3):
    """Plausible records, and between them records of a first fragment (an
    RPC header, so it can be guessed) and continuation fragments, one of
    which covers `span_chunks` whole chunks (0: it lies inside one chunk)."""
    rng = np.random.default_rng(seed + span_chunks)
    gen = FM.filler_records(rng, lo=28, hi=60)
    parts, pos = [], 0

    def add(b):
        nonlocal pos
        parts.append(b)
        pos += len(b)

    for r in range(rounds):
        for _ in range(int(rng.integers(2, 6))):
            add(next(gen))
        # first fragment: the header and a few bytes; then a short
        # continuation; then one starting right behind a chunk boundary that
        # covers span_chunks whole chunks; then the rest
        c1 = 44 + int(rng.integers(0, 8))
        c2 = c1 + int(rng.integers(1, 12))
        start3 = pos + 8 + c2                       # where the third fragment's mark would be
        if span_chunks:
            c2 += (-start3 % chunk) + 1             # ... moved to a chunk start + 1
        big = chunk * (span_chunks + 1) + 10 if span_chunks else 20
        body = FM.call(0x100 + r, _low(rng, c2 + big + int(rng.integers(5, 20)) - 40))[4:]
        add(fragment(body, [c1, c2, c2 + big]))
    for _ in range(4):
        add(next(gen))
    return b"".join(parts)


def whole_chunks_inside_a_fragment(buf, chunk):
    """The largest number of whole chunks lying inside one fragment."""
    off = frame_fragments(buf)[0].astype(np.int64)
    first_chunk = (off[:-1] + chunk - 1) // chunk      # first chunk starting at or after the fragment's mark
    inside = off[1:] // chunk - first_chunk
    return int(max(0, inside.max()))


@functools.lru_cache(maxsize=None)
def continuation_only_stream(chunk=EDGE_CHUNK, seed=5):
    """Records of many short continuation fragments (8..20 bytes each), so
    that whole chunks hold nothing but continuation starts."""
    rng = np.random.default_rng(seed)
    gen = FM.filler_records(rng, lo=28, hi=60)
    parts = [next(gen), next(gen)]
    for r in range(4):
        body = FM.call(0x200 + r, _low(rng, 6 * chunk))[4:]
        cuts, c = [], 48
        while c < len(body):
            cuts.append(c)
            c += int(rng.integers(4, 17))
        parts.append(fragment(body, cuts))
        parts.append(next(gen))
    return b"".join(parts)


def chunks_with_only_continuation_starts(buf, chunk):
    """Chunks that hold fragment starts, none of them a record's first fragment."""
    buf = bytes(buf)
    off = frame_fragments(buf)[0].astype(np.int64)[:-1]
    last = np.array([buf[int(p)] >> 7 for p in off], bool)
    first = np.concatenate(([True], last[:-1]))
    nch = (len(buf) + chunk - 1) // chunk
    starts = np.bincount(off // chunk, minlength=nch)
    firsts = np.bincount(off[first] // chunk, minlength=nch)
    return int(((starts > 0) & (firsts == 0)).sum())


@functools.lru_cache(maxsize=None)
def empty_fragments_stream(n=300, chunk=1024):
    """A record whose fragments are `n` 4-byte empty ones (more than 64
    starts in a chunk of 1024: the kept starts overflow) between plausible
    records."""
    rng = np.random.default_rng(9)
    gen = FM.filler_records(rng, lo=28, hi=60)
    body = FM.call(0x300, b"")[4:]
    rec = fragment(body, [40] + [40] * (n - 2))        # header, n - 2 empty ones, an empty last one
    return b"".join([next(gen), rec, next(gen), next(gen)])


def max_starts_in_a_chunk(buf, chunk):
    off = frame_fragments(buf)[0].astype(np.int64)[:-1]
    return int(np.bincount(off // chunk).max())


@functools.lru_cache(maxsize=None)
def straddle_stream(chunk=EDGE_CHUNK, seed=13):
    """Continuation fragments whose marks start at k * chunk + d for every d
    in -3..1."""
    rng = np.random.default_rng(seed)
    gen = FM.filler_records(rng, lo=28, hi=60)
    parts, pos = [], 0

    def add(b):
        nonlocal pos
        parts.append(b)
        pos += len(b)

    for d in (-3, -2, -1, 0, 1):
        add(next(gen))
        body = FM.reply(0x400 + d + 3, _low(rng, 3 * chunk))[4:]
        c1 = 30
        target = ((pos + 4 + c1) // chunk + 1) * chunk + d     # the second fragment's mark
        c1 = target - pos - 4
        add(fragment(body, [c1, c1 + 9]))
    add(next(gen))
    return b"".join(parts)


def straddle_offsets(buf, chunk):
    """The d in -3..1 for which a continuation fragment's mark lies at k * chunk + d."""
    buf = bytes(buf)
    off = frame_fragments(buf)[0].astype(np.int64)[:-1]
    last = np.array([buf[int(p)] >> 7 for p in off], bool)
    cont = off[1:][~last[:-1]]
    r = cont % chunk
    d = np.where(r > chunk // 2, r - chunk, r)
    return set(int(x) for x in d if -3 <= x <= 1)


@functools.lru_cache(maxsize=None)
def header_lookalike_stream(chunk=EDGE_CHUNK, seed=17):
    """Continuation fragments whose bodies are valid streams of plausible
    records: chunks inside them guess off the true chain."""
    rng = np.random.default_rng(seed)
    gen = FM.filler_records(rng, lo=28, hi=60)
    inner_gen = FM.filler_records(rng, first_xid=0x500, lo=28, hi=60)
    parts = [next(gen)]
    for r in range(3):
        inner = b"".join(next(inner_gen) for _ in range(12))
        body = FM.call(0x600 + r, inner)[4:]
        parts.append(fragment(body, [40, 40 + len(inner) // 2]))
        parts.append(next(gen))
        parts.append(next(gen))
    return b"".join(parts)


def plausible_first_fragment(buf, p):
    """frame.hip plausible_with<kFrag>: frame_model.plausible without the
    last-fragment bit (p + 16 <= len(buf))."""
    be = lambda q: _BE.unpack_from(buf, q)[0]
    h, mt, rv = be(p), be(p + 8), be(p + 12)
    want = (h & 0x7FFFFFFF) + 4
    if want < 24 or want > len(buf) - p:
        return False
    if mt == 0:
        return rv == 2 and want >= 44 and p + 36 <= len(buf) and be(p + 32) <= FM.MAX_AUTH_LEN
    if mt != 1 or rv > 1:
        return False
    if rv == 0:
        return want >= 28 and be(p + 20) <= FM.MAX_AUTH_LEN
    return be(p + 16) <= 1


def off_chain_guess_chunks(buf, chunk):
    """Chunks in which some position passes the fragment-mode start test but
    no fragment starts there."""
    buf = bytes(buf)
    starts = set(frame_fragments(buf)[0].astype(np.int64)[:-1].tolist())
    return len({p // chunk for p in range(len(buf) - 15) if p not in starts and plausible_first_fragment(buf, p)})


@functools.lru_cache(maxsize=None)
def big_continuation_stream(total=1 << 20, frag=256 << 10, seed=19):
    """About `total` bytes: records of a few KiB to `frag`-sized continuation
    fragments (the default chunk is 64 KiB: four whole chunks inside each)."""
    rng = np.random.default_rng(seed)
    gen = FM.filler_records(rng)
    parts, pos = [], 0
    while pos < total:
        for _ in range(int(rng.integers(1, 40))):
            parts.append(next(gen))
            pos += len(parts[-1])
        body = FM.call(0x700, rng.bytes(2 * frag + int(rng.integers(0, 5000))))[4:]
        parts.append(fragment(body, [int(rng.integers(44, 3000)), frag, 2 * frag]))
        pos += len(parts[-1])
    return b"".join(parts)


# ---------------------------------------------------------------------------
# streams for the copy
# ---------------------------------------------------------------------------
ALIGN_LENS = (0, 1, 3, 15, 16, 17, 33)


@functools.lru_cache(maxsize=None)
def alignment_stream(seed=23, reps=3):
    """Two-fragment records with body lengths (a, b) over every pair of
    ALIGN_LENS, `reps` times in shuffled order."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(reps):
        pairs = [(a, b) for a in ALIGN_LENS for b in ALIGN_LENS]
        rng.shuffle(pairs)
        for a, b in pairs:
            parts.append(fragment(rng.bytes(a + b), [a]))
    return b"".join(parts)


def alignment_coverage(buf, shifts=range(16)):
    """{(source address mod 16, destination address mod 16)} over the second
    fragments' bodies, the wire at a 16-byte aligned address and `out` at
    shift past one, for every shift."""
    fo = frame_fragments(buf)[0]
    m = defragment(buf, fo)
    fo = fo.astype(np.int64)
    src = fo[1:-1:2] + 4                                  # second fragment of record i: fragment 2i + 1
    first_len = fo[1:-1:2] - fo[0:-2:2] - 4
    dst = m["rec_off"][:-1].astype(np.int64) + 4 + first_len
    return {(int(s) % 16, (int(d) + sh) % 16) for s, d in zip(src, dst) for sh in shifts}


@functools.lru_cache(maxsize=None)
def shapes_stream(which, seed=29):
    rng = np.random.default_rng(seed)
    if which == "tiny":
        # many fragments inside one 16-byte output chunk: bodies of 0..3 bytes
        recs = []
        for _ in range(40):
            k = int(rng.integers(2, 30))
            lens = rng.integers(0, 4, k)
            body = rng.bytes(int(lens.sum()))
            recs.append(fragment(body, np.cumsum(lens)[:-1].tolist()))
        return b"".join(recs)
    if which in ("frags65", "frags200"):
        k = 65 if which == "frags65" else 200
        lens = rng.integers(0, 40, k)
        body = rng.bytes(int(lens.sum()))
        return FM.reply28(1) + fragment(body, np.cumsum(lens)[:-1].tolist()) + FM.reply28(2)
    if which == "huge":
        # one fragment larger than several 8 KiB output tiles
        body = rng.bytes(100_000)
        return FM.reply28(1) + fragment(body, [7, 7 + 70_001]) + FM.reply28(2)
    if which == "multi_first":
        return fragment(rng.bytes(100), [10, 50]) + FM.reply28(3) + FM.opaque(rng.bytes(9))
    if which == "multi_last":
        return FM.opaque(rng.bytes(9)) + FM.reply28(3) + fragment(rng.bytes(100), [10, 50])
    if which == "empty":
        # an empty record as one fragment, as two, between others and at the ends
        e1, e2 = _BE.pack(LAST), _BE.pack(0) + _BE.pack(LAST)
        return e1 + FM.reply28(4) + e2 + e1 + fragment(rng.bytes(20), [5]) + e2
    raise KeyError(which)


SHAPES = ("tiny", "frags65", "frags200", "huge", "multi_first", "multi_last", "empty")


TILE = 8192          # defrag.hip kDfTile: output bytes per wave and step
STAGE = 128          # defrag.hip kDfStage: fragments of a tile kept in LDS


def fragment_out_offsets(buf):
    """Where every fragment's bytes start in the reassembled stream (a
    record's first fragment: at the record's mark)."""
    buf = bytes(buf)
    fo = frame_fragments(buf)[0].astype(np.int64)
    out, pos, first = [], 0, True
    for j in range(len(fo) - 1):
        out.append(pos)
        pos += int(fo[j + 1] - fo[j]) - (0 if first else 4)
        first = bool(buf[int(fo[j])] & 0x80)
    return np.array(out, np.int64)


@functools.lru_cache(maxsize=None)
def tile_boundary_stream(kind, origin, seed=37):
    """Fragments piled up where an output tile begins (out at `origin` bytes
    past a 16-byte aligned address: tile 1's first byte is out[TILE - origin]).
    A record's first fragment ends right there; then come
      'search' : 300 empty continuation fragments;
      'slide'  : 100 empty ones, then 60 of one byte;
      'spill'  : 100 empty ones, then 200 of one byte;
    and a last fragment of 3000 bytes, between plain records.

    The stream is three tiles long, so at the default grid every tile is the
    first of its wave's run: its first fragment is found by the search in
    global memory, which steps over the empty ones, and the staged window
    starts there. What these streams reach is that search landing on the last
    of many equal positions, and for 'spill' a first tile of more fragments
    than the window (copied from global memory); 'search' and 'slide' do not
    take the copy's window-restart branches. tile_run_stream below puts the
    same pile-ups on a tile that is carried, and tests/test_gpu_tile_runs.py
    runs them in one workgroup, where they do."""
    rng = np.random.default_rng(seed)
    empties, ones = {"search": (300, 0), "slide": (100, 60), "spill": (100, 200)}[kind]
    at = TILE - origin                       # out offset of tile 1's first byte
    head = FM.opaque(rng.bytes(5000))
    first_body = at - len(head) - 4
    body = rng.bytes(first_body + ones + 3000)
    cuts = [first_body] * (empties + 1) + [first_body + i for i in range(1, ones + 1)]
    return head + fragment(body, cuts) + FM.opaque(rng.bytes(9000)) + FM.reply28(5)


def tile_run_stream(kind, ntiles, origin, seed=41):
    """-> (stream, entries): tile_walk_model.layout(kind, ntiles, origin) as
    fragments — an entry of no output is an empty continuation fragment, a
    short one a continuation of one byte, and about every other ordinary entry
    starts a new record (its four mark bytes count as its output). The
    positions of the walk are fragment_out_offsets(stream) and the total."""
    import tile_walk_model as TW
    entries, _ = TW.layout(kind, ntiles, origin)
    rng = np.random.default_rng(seed + ntiles)
    parts, cur = [], None
    for i, (ln, what) in enumerate(entries):
        if i == 0 or (what == "fill" and ln >= 4 and rng.random() < 0.5):
            if cur is not None:
                parts.append(fragment(rng.bytes(sum(cur)), np.cumsum(cur)[:-1].tolist()))
            cur = [ln - 4]
        else:
            cur.append(ln)
    parts.append(fragment(rng.bytes(sum(cur)), np.cumsum(cur)[:-1].tolist()))
    return b"".join(parts), entries


def fragments_per_record(buf):
    buf = bytes(buf)
    off = frame_fragments(buf)[0].astype(np.int64)[:-1]
    last = np.array([buf[int(p)] >> 7 for p in off], bool)
    ends = np.nonzero(last)[0]
    return np.diff(np.concatenate(([-1], ends)))


@functools.lru_cache(maxsize=None)
def pending_stream(seed=31):
    """Complete records, then three fragments of a record whose last
    fragment has not arrived."""
    rng = np.random.default_rng(seed)
    head = FM.reply28(1) + fragment(rng.bytes(300), [100, 200]) + FM.reply28(2)
    tail = fragment(rng.bytes(90), [20, 50, 90])           # four fragments, the last one empty ...
    return head + tail[:-4], len(head)                     # ... and missing
