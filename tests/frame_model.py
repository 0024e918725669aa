"""Host model of the device framer's observable state, and the builders of
the streams the framer edge tests use (tests/test_frame_model.py on the CPU,
tests/test_gpu_frame_edges.py on the GPU).

Not a test file and not product code: plain numpy / Python restating the
rules written down in onc-rpc_amd/csrc/frame.hip's comments — the caller's
expected_message_len loop (the true chain), the plausibility test of a
record start, the per-chunk guess, and what a lane of frame_chunks derives
from a guess (exit chunk, stop, verification failure). The builders use it
to prove, on the CPU, that each stream has the property it was built for.
"""
from __future__ import annotations

import functools
import struct

import numpy as np

OK, INCOMPLETE_MESSAGE, INCOMPLETE_HEADER, FRAGMENTED = 0, 1, 2, 3
MAX_AUTH_LEN = 200
_BE = struct.Struct(">I")


def _be(buf, p):
    return _BE.unpack_from(buf, p)[0]


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def true_starts(buf, max_records=None):
    """The serial expected_message_len loop over `buf`:
    (starts int64[n], stop position, status, aux0, aux1) — the record starts,
    where the loop ended and why (oracle.frame_stream's rec_off[:n],
    consumed, status, aux0, aux1)."""
    buf = bytes(buf)
    n_max = len(buf) // 4 + 1 if max_records is None else max_records
    ln = len(buf)
    starts = []
    p, st, a0, a1 = 0, OK, 0, 0
    while p < ln and len(starts) < n_max:
        if ln - p < 4:
            st = INCOMPLETE_HEADER
            break
        h = _be(buf, p)
        if not h & 0x80000000:
            st = FRAGMENTED
            break
        want = (h & 0x7FFFFFFF) + 4
        if ln - p < want:
            st, a0, a1 = INCOMPLETE_MESSAGE, ln - p, want & 0xFFFFFFFF
            break
        starts.append(p)
        p += want
    return np.array(starts, np.int64), p, st, a0, a1


def plausible(buf, p):
    """frame.hip plausible_with: does a record start at p look like an
    ONC-RPC message (p + 16 <= len(buf))."""
    ln = len(buf)
    h, mt, rv = _be(buf, p), _be(buf, p + 8), _be(buf, p + 12)
    want = (h & 0x7FFFFFFF) + 4
    if not h & 0x80000000 or want < 24 or want > ln - p:
        return False
    if mt == 0:
        return rv == 2 and want >= 44 and _be(buf, p + 32) <= MAX_AUTH_LEN
    if mt != 1 or rv > 1:
        return False
    if rv == 0:
        return want >= 28 and _be(buf, p + 20) <= MAX_AUTH_LEN
    return _be(buf, p + 16) <= 1


def candidates(buf):
    """Positions passing frame_guess's byte filter (high bit set, three zero
    bytes at +8..+10) with p + 16 <= len, ascending."""
    a = np.frombuffer(bytes(buf), np.uint8)
    m = len(a) - 15
    if m <= 0:
        return np.zeros(0, np.int64)
    c = (a[:m] >= 0x80) & (a[8:m + 8] == 0) & (a[9:m + 9] == 0) & (a[10:m + 10] == 0)
    return np.nonzero(c)[0].astype(np.int64)


def guesses(buf, chunk):
    """Per chunk the first position p in it with p + 16 <= len, p plausible,
    and p's claimed end q either within 16 bytes of the end (q + 16 > len)
    or plausible itself; -1 where there is none. Chunk 0 guesses 0."""
    buf = bytes(buf)
    ln = len(buf)
    nch = (ln + chunk - 1) // chunk
    g = np.full(nch, -1, np.int64)
    if nch:
        g[0] = 0
    for p in candidates(buf).tolist():
        t = p // chunk
        if g[t] >= 0:
            continue
        if plausible(buf, p):
            q = p + (_be(buf, p) & 0x7FFFFFFF) + 4
            if q + 16 > ln or plausible(buf, q):
                g[t] = p
    return g


def _chase(buf, p, lim):
    """frame.hip chase: the chain from p while p < lim -> (x, count, st)
    with st -1 when the chain leaves [.., lim) with more to come."""
    ln = len(buf)
    cnt, st = 0, -1
    while p < lim:
        if ln - p < 4:
            st = INCOMPLETE_HEADER
            break
        h = _be(buf, p)
        if not h & 0x80000000:
            st = FRAGMENTED
            break
        want = (h & 0x7FFFFFFF) + 4
        if ln - p < want:
            st = INCOMPLETE_MESSAGE
            break
        cnt += 1
        p += want
    if st == -1 and p >= ln:
        st = OK
    return p, cnt, st


def chunk_flags(buf, chunk):
    """What frame_chunks sees per chunk, as a dict of arrays (one entry per
    chunk):
      g         the guess (-1: none)
      on_chain  the guess is a true record start
      starts    true record starts in the chunk
      exit      the chunk the guess's chain leaves to (-1: no guess, or the
                chain ends in this chunk)
      stop_st   status with which the guess's chain ends in this chunk (-1:
                it does not), stop_pos where
      fail      the verification fails: the chain lands off the landing
                chunk's guess, or jumps over a guessed chunk
    plus 'chain' = true_starts(buf)."""
    buf = bytes(buf)
    ln = len(buf)
    g = guesses(buf, chunk)
    nch = len(g)
    chain = true_starts(buf)
    ts = chain[0]
    starts = np.bincount(ts // chunk, minlength=nch).astype(np.int64) if len(ts) else np.zeros(nch, np.int64)
    on_chain = np.zeros(nch, bool)
    on_chain[g >= 0] = np.isin(g[g >= 0], ts)
    ex = np.full(nch, -1, np.int64)
    stop_st = np.full(nch, -1, np.int64)
    stop_pos = np.full(nch, -1, np.int64)
    fail = np.zeros(nch, bool)
    guessed = np.nonzero(g >= 0)[0]
    for i, t in enumerate(guessed.tolist()):
        x, _, st = _chase(buf, int(g[t]), min((t + 1) * chunk, ln))
        if st != -1:
            stop_st[t], stop_pos[t] = st, x
            continue
        j = x // chunk
        ex[t] = j
        nxt = int(guessed[i + 1]) if i + 1 < len(guessed) else nch
        fail[t] = j >= nch or g[j] != x or nxt < j
    return {"g": g, "on_chain": on_chain, "starts": starts, "exit": ex, "stop_st": stop_st, "stop_pos": stop_pos,
            "fail": fail, "chain": chain}


# ---------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------
def reply28(xid):
    """The smallest plausible Reply (accepted, AUTH_NONE verifier, Success)."""
    return struct.pack(">7I", 0x80000018, xid, 1, 0, 0, 0, 0)


def reply(xid, payload=b""):
    return struct.pack(">7I", 0x80000000 | (24 + len(payload)), xid, 1, 0, 0, 0, 0) + payload


def call(xid, payload=b""):
    """A plausible Call with AUTH_NONE credential and verifier (44 bytes + payload)."""
    return struct.pack(">11I", 0x80000000 | (40 + len(payload)), xid, 0, 2, 1, 1, 1, 0, 0, 0, 0) + payload


def opaque(body):
    """A record that is only a mark and bytes."""
    return struct.pack(">I", 0x80000000 | len(body)) + body


def _low_bytes(rng, n):
    """n bytes with the high bit clear: none passes the candidate filter."""
    return rng.integers(0, 128, n, dtype=np.uint8).tobytes()


def filler_records(rng, first_xid=1, lo=28, hi=300):
    """Endless plausible records of lo..hi bytes (Calls and Replies, small
    xids, payload bytes with the high bit clear: only the marks are
    candidates, so every guess verifies)."""
    xid = first_xid
    while True:
        n = int(rng.integers(lo, hi + 1))
        if n >= 44 and rng.random() < 0.5:
            yield call(xid & 0x7F7F, _low_bytes(rng, n - 44))
        else:
            yield reply(xid & 0x7F7F, _low_bytes(rng, n - 28))
        xid += 1


def nested_call(xid, inner, gap=0):
    """An outer Call whose payload is the stream `inner`, then `gap` bytes
    with the high bit clear (gap 0: the inner chain lands on the record after
    the outer one; gap 1..3: it stops there as Fragmented)."""
    return call(xid, inner + b"\x01" * gap)


# ---------------------------------------------------------------------------
# (a) starts per chunk around kStartsCap
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def replies_stream(n=4000):
    return b"".join(reply28(i & 0x7F7F) for i in range(n))


@functools.lru_cache(maxsize=None)
def opaque16_stream(first_len, n=3000, seed=7):
    """16-byte opaque records (mark + 12 random bytes) behind a first record
    of first_len bytes; every 97th record is 32 bytes long and every 89th is
    split into two of 8, so 1024-byte chunks hold 63, 64 or 65 starts."""
    rng = np.random.default_rng(seed + first_len)
    parts = [opaque(rng.bytes(first_len - 4))]
    for i in range(1, n):
        if i % 97 == 0:
            parts.append(opaque(rng.bytes(28)))
        elif i % 89 == 0:
            parts += [opaque(rng.bytes(4)), opaque(rng.bytes(4))]
        else:
            parts.append(opaque(rng.bytes(12)))
    return b"".join(parts)


# ---------------------------------------------------------------------------
# (c) marks straddling chunk boundaries
# ---------------------------------------------------------------------------
STRADDLE_D = (-3, -2, -1, 0, 1)


@functools.lru_cache(maxsize=None)
def straddle_stream(chunk, kind, rounds=6):
    """Records laid so that, for every d in STRADDLE_D, some record's mark
    starts at k * chunk + d: before each target the previous record is
    stretched to end exactly there. kind: 'plausible' (Calls / Replies) or
    'opaque'."""
    rng = np.random.default_rng(chunk + len(kind))
    parts, pos, xid = [], 0, 1
    floor = 28 if kind == "plausible" else 4

    def rec(n):
        nonlocal xid
        xid += 1
        if kind == "opaque":
            return opaque(rng.bytes(n - 4))
        return call(xid, _low_bytes(rng, n - 44)) if n >= 44 else reply(xid, _low_bytes(rng, n - 28))

    for _ in range(rounds):
        for d in STRADDLE_D:
            k = (pos + 2 * floor + 70) // chunk + 2
            target = k * chunk + d
            mid = int(rng.integers(floor, floor + 30))
            for n in (mid, target - pos - mid):
                parts.append(rec(n))
                pos += n
            n = int(rng.integers(floor, floor + 40))
            parts.append(rec(n))
            pos += n
    return b"".join(parts)


def straddle_offsets(buf, chunk):
    """The d in STRADDLE_D for which some true start lies at k * chunk + d, k >= 1."""
    ts = true_starts(buf)[0]
    ts = ts[ts >= chunk - 3]
    r = ts % chunk
    d = np.where(r > chunk // 2, r - chunk, r)
    return set(int(x) for x in d if -3 <= x <= 1)


# ---------------------------------------------------------------------------
# (e) nested streams and stale flags
# ---------------------------------------------------------------------------
def _take(gen, nbytes):
    """Records from gen, up to nbytes in all."""
    parts, pos = [], 0
    while True:
        r = next(gen)
        if pos + len(r) > nbytes:
            break
        parts.append(r)
        pos += len(r)
    return b"".join(parts)


def _decoy(rng, xid, start, chunk, inner_len, gap, lo, hi, cleared=True):
    """An outer Call at stream offset `start` whose payload is an inner
    stream of about inner_len bytes, then `gap` bytes. With a gap, the inner
    stream closes with two 28-byte Replies placed so that both and the gap
    position G lie in one chunk: that chunk's guess is then the first of the
    two, and its chain stops at G (a false stop). cleared: G is `gap` bytes
    before a chunk boundary, so the outer record ends on the boundary and the
    false stop's chunk is one the record jumps over (the walk clears its
    guess); else G % chunk == 56 and the outer record ends in the false
    stop's chunk (the walk re-chases it)."""
    inner = _take(filler_records(rng, first_xid=0x100, lo=lo, hi=hi), inner_len)
    if gap:
        want = chunk - gap if cleared else 56
        s = (want - (start + 44 + len(inner) + 56)) % chunk
        if s and s < 28:
            s += chunk
        if s:
            for n in ((s,) if s < 56 else (28, s - 28)):       # none covers a whole 64-byte chunk
                inner += reply(0x55, b"\x03" * (n - 28))
        inner += reply28(0x57) + reply28(0x58)
        assert (start + 44 + len(inner)) % chunk == want >= 56
    return nested_call(xid, inner, gap)


@functools.lru_cache(maxsize=None)
def nested_stream(chunk, inner_len, variant, placement, gap, seed=11):
    """(stream, info): plausible filler records around an outer Call whose
    payload is a valid stream of about inner_len bytes (3 chunks or more).
    variant 1: the inner stream fills the payload, so the inner chain lands
    on the record after the outer one (gap 0); variants 2 and 3: it ends `gap`
    (1, 2 or 3) bytes short, so the inner chain stops there as Fragmented — in a
    chunk the outer record jumps over (2: the walk clears that chunk's guess)
    or in the chunk the outer record ends in (3: the walk re-chases it).
    placement 'first': the outer record is the stream's first verification
    failure; 'later': before it, a record longer than a chunk is followed by
    an implausible one, so that chain lands where no chunk guessed (an
    earlier failure). info: outer record start and end, gap position."""
    assert gap == 0 if variant == 1 else gap in (1, 2, 3)
    rng = np.random.default_rng(seed + chunk + variant + 7 * gap)
    lo, hi = (28, 300) if chunk >= 1024 else (28, 60)
    gen = filler_records(rng, lo=lo, hi=hi)
    parts = [_take(gen, 3 * chunk + 100)]
    if placement == "later":
        parts.append(call(0x3333, _low_bytes(rng, chunk + 10)))
        parts.append(opaque(_low_bytes(rng, 16)))
        parts.append(_take(gen, 2 * chunk + 50))
    start = sum(len(p) for p in parts)
    outer = _decoy(rng, 0x4444, start, chunk, inner_len, gap, lo, hi, cleared=variant == 2)
    parts.append(outer)
    parts.append(_take(gen, 4 * chunk + 77))
    buf = b"".join(parts)
    end = start + len(outer)
    return buf, {"outer": start, "end": end, "gap": gap, "gap_pos": end - gap if gap else None, "variant": variant}


def check_nested(buf, chunk, info, placement):
    """The preconditions of a nested stream, from the model; returns a
    summary for the logs."""
    f = chunk_flags(buf, chunk)
    ts, stop, st = f["chain"][0], f["chain"][1], f["chain"][2]
    assert st == OK and stop == len(buf)
    assert info["outer"] in ts and info["end"] in ts
    t0, t1 = info["outer"] // chunk, info["end"] // chunk
    inside = np.arange(t0 + 1, t1)
    assert len(inside) >= 3, "the payload spans at least 3 chunks"
    assert (f["g"][inside] >= 0).all() and not f["on_chain"][inside].any(), "off-chain guesses inside the payload"
    assert f["on_chain"][(f["g"] >= 0) & ((np.arange(len(f["g"])) <= t0) | (np.arange(len(f["g"])) >= t1 + 1))].all()
    fails = np.nonzero(f["fail"])[0]
    # the chunk whose chain carries the outer record jumps over guessed chunks
    carrier = int(np.nonzero((f["g"] >= 0) & (f["g"] <= info["outer"]))[0][-1])
    assert f["fail"][carrier]
    if placement == "first":
        assert fails[0] == carrier
    else:
        assert fails[0] < carrier
    stops = np.nonzero(f["stop_st"] >= 0)[0]
    if info["gap"]:
        ts_ = info["gap_pos"] // chunk
        assert f["stop_st"][ts_] == FRAGMENTED and f["stop_pos"][ts_] == info["gap_pos"] and not f["on_chain"][ts_]
        assert t0 < ts_ < t1 if info["variant"] == 2 else ts_ == t1, "in a jumped-over chunk / the landing chunk"
        assert stops[0] == ts_ and ts_ > fails[0], "the false stop is the first stop flag, after the first failure"
        assert len(stops) == 2 and stops[1] > t1, "and the only other one is the buffer's end"
    else:
        assert len(stops) == 1 and stops[0] > t1
    return {"chunks": len(f["g"]), "carrier": carrier, "inside": (int(inside[0]), int(inside[-1])),
            "fails": fails.tolist(), "stops": stops.tolist()}


# ---------------------------------------------------------------------------
# (f) flag hierarchy
# ---------------------------------------------------------------------------
HIER_CHUNK = 64
HIER_LAYOUTS = {
    # decoy chunks, opaque (chunk, bytes) or None, the real Fragmented stop's chunk
    "plain": {"decoys": (10, 70_000, 70_300), "opaque": None, "stop": 140_000},
    "opaque": {"decoys": (10, 125_000, 125_300), "opaque": (40_000, 5 << 20), "stop": 165_000},
}
HIER_BYTES = 10 * (1 << 20) + (1 << 19)


@functools.lru_cache(maxsize=None)
def hier_stream(name, seed=23):
    """(stream, info): about 10.5 MiB of 28..300-byte plausible records (more
    than 2.5 x 65536 chunks of 64 bytes) with three decoys a few chunks long (outer
    Calls carrying an inner stream; the second ends 1..3 bytes short: a false
    stop), optionally a 5 MiB opaque random record, and a cleared
    last-fragment bit (the real stop), at HIER_LAYOUTS[name]'s chunks."""
    lay = HIER_LAYOUTS[name]
    chunk = HIER_CHUNK
    rng = np.random.default_rng(seed)
    gen = filler_records(rng)
    items = [(c * chunk, "decoy", i) for i, c in enumerate(lay["decoys"])]
    if lay["opaque"]:
        items.append((lay["opaque"][0] * chunk, "opaque", lay["opaque"][1]))
    items.append((lay["stop"] * chunk, "stop", 0))
    items.sort()
    parts, pos, info = [], 0, {"decoys": [], "gap_pos": None}

    def fill_to(target):
        nonlocal pos
        while pos < target:
            r = next(gen)
            parts.append(r)
            pos += len(r)

    for target, what, arg in items:
        fill_to(target)
        if what == "decoy":
            gap = 2 if arg == 1 else 0
            r = _decoy(rng, 0x4000 + arg, pos, chunk, 260, gap, 28, 40)
            info["decoys"].append((pos, pos + len(r)))
            if gap:
                info["gap_pos"] = pos + len(r) - gap
        elif what == "opaque":
            r = opaque(rng.bytes(arg))
            info["opaque"] = (pos, pos + len(r))
        else:
            r = reply(0x99, b"\x05" * 40)
            r = bytes([r[0] & 0x7F]) + r[1:]
            info["stop"] = pos
        parts.append(r)
        pos += len(r)
    fill_to(HIER_BYTES)
    return b"".join(parts), info


def check_hier(buf, info, name):
    lay = HIER_LAYOUTS[name]
    chunk = HIER_CHUNK
    f = chunk_flags(buf, chunk)
    nch = len(f["g"])
    assert nch > 2.5 * 65536
    ts, stop, st = f["chain"][0], f["chain"][1], f["chain"][2]
    assert (stop, st) == (info["stop"], FRAGMENTED)
    ts_chunk = info["stop"] // chunk
    assert abs(ts_chunk - lay["stop"]) <= 8 and ts_chunk >> 16 == 2
    idx = np.arange(nch)
    before = idx <= ts_chunk
    off = np.nonzero((f["g"] >= 0) & ~f["on_chain"] & (idx < ts_chunk))[0]
    in_decoy = np.zeros(nch, bool)
    carriers = []
    for want, (a, b) in zip(lay["decoys"], info["decoys"]):
        assert a in ts and b in ts
        t0, t1 = a // chunk, b // chunk
        assert abs(t0 - want) <= 8 and t1 - t0 >= 3
        inside = np.arange(t0 + 1, t1)
        assert len(inside) >= 2 and (f["g"][inside] >= 0).all() and not f["on_chain"][inside].any()
        in_decoy[t0:t1 + 1] = True
        c = int(np.nonzero((f["g"] >= 0) & (f["g"] <= a))[0][-1])
        assert f["fail"][c]
        carriers.append(c)
    assert in_decoy[off].all(), "no off-chain guess outside the decoys (before the real stop)"
    assert carriers[0] >> 16 == 0 and carriers[1] >> 16 == 1 and carriers[2] >> 16 == 1
    assert carriers[1] >> 8 != carriers[2] >> 8
    fails = np.nonzero(f["fail"] & before)[0]
    # the failures before the real stop: the three decoys, and the chunks
    # whose chain lands on an implausible start in a later chunk (the cleared
    # mark; the opaque record)
    land = [ts_chunk] + ([info["opaque"][0] // chunk] if lay["opaque"] else [])
    extra = [int(t) for t in fails if t not in carriers]
    assert all(any(0 <= e - t <= 8 for e in land) for t in extra), extra
    gs = info["gap_pos"] // chunk
    assert f["stop_st"][gs] == FRAGMENTED and f["stop_pos"][gs] == info["gap_pos"] and in_decoy[gs]
    stops = np.nonzero((f["stop_st"] >= 0) & before)[0]
    assert stops[0] == gs and all(t >= ts_chunk - 8 for t in stops[1:])
    assert gs < info["decoys"][1][1] // chunk, "the false stop's chunk is jumped over: the walk clears it"
    if lay["opaque"]:
        a, b = info["opaque"]
        assert a in ts and b in ts and b - a > 5 << 20
        inside = np.arange(a // chunk + 1, b // chunk)
        assert not (f["g"][inside] >= 0).any(), "no guess inside the opaque record"
    return {"chunks": nch, "carriers": carriers, "false_stop": int(gs), "real_stop": int(ts_chunk),
            "fails": fails.tolist(), "records": len(ts)}


# ---------------------------------------------------------------------------
# (g) tiny buffers and zero-length records; (h) the larger streams
# ---------------------------------------------------------------------------
def tiny_buffers():
    return [b"\x80", b"\x80\x00", b"\x80\x00\x00", b"\x80\x00\x00\x00", b"\x00\x00\x00\x00", b"\x7f\xff\xff\xff",
            b"\x00\x00\x00\x18" + reply28(1)[4:], b"\xff\xff\xff\xff", b"\xff\xff\xff\xff" + b"\x00" * 40,
            reply28(1) + b"\xff\xff\xff\xff" + b"\x01" * 9, b"\x80\x00\x00\x00" * 3 + b"\x80\x00"]


def zero_records(n=4000):
    return b"\x80\x00\x00\x00" * n


@functools.lru_cache(maxsize=None)
def big_filler_stream(nbytes, seed=31):
    rng = np.random.default_rng(seed)
    gen = filler_records(rng)
    parts, pos = [], 0
    while pos < nbytes:
        r = next(gen)
        parts.append(r)
        pos += len(r)
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def mixed_stream(n, seed, pmin, pmax):
    """The oracle's encoding of synth.mixed(n, seed, pmin, pmax): a valid
    stream with random xids and payloads (candidates anywhere)."""
    import oracle_ffi
    import onc_rpc_amd.synth as S
    wire, _, st, _ = oracle_ffi.encode_batch(S.mixed(n, seed=seed, pmin=pmin, pmax=pmax))
    assert not st.any()
    return wire


def edge_stream():
    """(b): about 2000 mixed records, payloads 0..600."""
    return mixed_stream(2000, 41, 0, 600)


def cut_stream():
    """(d): about 200 mixed records, 12..20 KB."""
    return mixed_stream(200, 43, 0, 100)


NESTED_CASES = [(chunk, inner, variant, placement, gap)
                for chunk, inner in ((65536, 300_000), (1024, 20_000))
                for variant in (1, 2, 3) for placement in ("first", "later")
                for gap in ((0,) if variant == 1 else (1, 2, 3))]


def starts_histogram(buf, chunk):
    """{starts in a chunk: number of such chunks} of the true chain."""
    ts = true_starts(buf)[0]
    nch = (len(buf) + chunk - 1) // chunk
    h = np.bincount(np.bincount(ts // chunk, minlength=nch))
    return {int(k): int(v) for k, v in enumerate(h) if v}
