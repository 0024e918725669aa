"""The inputs of the scan-round tests, shared by tests/test_gpu_scan_rounds.py
(the GPU against the host models) and tests/test_scan_rounds_model.py (the
proof on the CPU that those cases bite), so that both see the same arrays.

Six calls reduce per-block or per-tile counts in ONE workgroup that walks the
counts in rounds and carries a running aggregate from a round to the next:

  call                 kernel               a round covers
  onc_fragment_iov     fragiov_blkscan      256 blocks x 256 records   = R_PLAN
  onc_piece_offsets    gath_blkscan         256 blocks x 256 pieces    = R_PLAN
  onc_payload_slots    pay_blkscan          256 blocks x 256 records   = R_PLAN
  onc_route_calls      route_scan_bins      256 tiles x 1024 records   = R_ROUTE
  onc_group_by_conn    group_scan_digits    256 tiles x 1024 items     = R_GROUP
  onc_match_replies    match_scan           1024 tiles x 1024 entries  = R_MATCH
                       (and its class sums, a stride of 1024 record tiles)
The last three walk their rounds in one loop, scan_bin_row of
onc-rpc_amd/csrc/partition.h, at the round lengths their own files assert.

The builders here make inputs whose counts reach a second and a third round.
The lost_carry_* functions construct, from a model's right result, what the
call would have written had that workgroup dropped its carry: every element a
round k > 0 owns is short of the totals of the rounds before k, and the batch
totals are the last round's alone. Not a test file and not product code.
"""
from __future__ import annotations

import functools

import numpy as np

import fragment_iov_model as V
import gather_model as G
import group_model as GM
import onc_rpc_amd.layout as L
import route_model as RM

R_PLAN = 256 * 256            # tile_walk.h kCopyThreads blocks of kCopyThreads records
R_ROUTE = 256 * 1024          # route.hip kRtScanThreads tiles of kRouteTile records
R_GROUP = 256 * 1024          # group.hip kGrFlat tiles of kGroupTile items
R_MATCH = 1024 * 1024         # match.hip kMtThreads tiles of kMatchTile entries (or records)
TILE = 1024                   # records / items / entries per tile of route, group and match
SENT = 0xA5
U32 = 0xFFFFFFFF

PLAN_SIZES = (R_PLAN, R_PLAN + 1, R_PLAN + 257, 2 * R_PLAN + 1)
ROUTE_SIZES = (R_ROUTE, R_ROUTE + 1, R_ROUTE + 1025, 2 * R_ROUTE + 1)
GROUP_SIZES = (R_GROUP + 1, 2 * R_GROUP + 1)


def rounds(n, R):
    """How many rounds the scan of n elements takes."""
    return (n + R - 1) // R


# ---------------------------------------------------------------------------
# a scan that starts every round at zero
# ---------------------------------------------------------------------------
def drop_carry(prefix, R):
    """prefix[i] = the total of the elements before i, prefix[n] = the batch
    (n + 1 entries). -> the same array from a scan whose every round starts at
    zero: entry i of round k is short of prefix[k R], entry n is the last
    round's total alone. With one round it is the array itself."""
    p = np.asarray(prefix)
    n = len(p) - 1
    out = p.copy()
    i = np.arange(n)
    out[:n] = p[:n] - p[i // R * R]
    out[n] = p[n] - p[(n - 1) // R * R] if n else p[n]
    return out


def last_round(n, R):
    """The elements of the last round, as a slice."""
    return slice((n - 1) // R * R, n)


def partition_without_carry(key, nb, R):
    """The stable partition of route_scatter / group_scatter over nb bins,
    with the per-bin scan of the tile counts (rounds of R items) starting
    every round at zero -> (dest[n], first[nb + 1]): an item lands at first[its
    bin] + its rank among the items of its bin in its own round; first is the
    scan of the last round's totals, which is all the carry-less scan keeps."""
    key = np.asarray(key, np.int64)
    n = len(key)
    total = np.bincount(key[last_round(n, R)], minlength=nb) if n else np.zeros(nb, np.int64)
    first = np.concatenate(([0], np.cumsum(total))).astype(np.int64)
    dest = np.zeros(n, np.int64)
    for lo in range(0, n, R):
        k = key[lo:lo + R]
        o = np.argsort(k, kind="stable")
        cnt = np.bincount(k, minlength=nb)
        rank = np.empty(len(k), np.int64)
        rank[o] = np.arange(len(k)) - (np.cumsum(cnt) - cnt)[k[o]]
        dest[lo:lo + R] = first[k] + rank
    return dest, first


def scatter(dest, values, n, fill):
    """values[i] written to out[dest[i]] in item order (a later item wins, a
    destination outside [0, n) is dropped), `fill` where nothing lands."""
    out = np.full(n, fill, dtype=np.asarray(values).dtype) if np.isscalar(fill) else np.tile(fill, n)
    ok = (dest >= 0) & (dest < n)
    out[dest[ok]] = np.asarray(values)[ok]
    return out


# ---------------------------------------------------------------------------
# onc_fragment_iov
# ---------------------------------------------------------------------------
FIV_F = 9
FIV_LIMITS = (1, 3, 9, 16, 100, V.MAX_FRAG_LIMIT, 0, 0x80000000)


@functools.lru_cache(maxsize=None)
def fiv_case(n, per_record=False):
    """-> (iov, rec_max_frag or None): n entries in the style of
    fragment_iov_model.short_records — records of 4..40 bytes, the header 4..L
    of them, so that at max_frag 9 most split — and, one in sixteen each,
    placeholders of no bytes and failing records (a header shorter than a
    mark: ENC_BAD_DESCRIPTOR). Both kinds stand on both sides of record
    R_PLAN, and the records R_PLAN - 1 and R_PLAN themselves take pieces.
    per_record: a limit per record, the invalid values 0 and 2^31 among them
    on both sides of R_PLAN too."""
    rng = np.random.default_rng(9000 + n + (1 if per_record else 0))
    i = np.arange(n)
    ln = rng.integers(4, 41, n)
    h = rng.integers(4, ln + 1)
    p = ln - h
    kind = rng.integers(0, 16, n)                    # 0: a placeholder, 1: a failing record
    for at, k in ((R_PLAN - 3, 0), (R_PLAN - 2, 1), (R_PLAN - 1, 9), (R_PLAN, 9), (R_PLAN + 1, 0), (R_PLAN + 2, 1)):
        if at < n:
            kind[at] = k
    h[kind == 0], p[kind == 0] = 0, 0
    h[kind == 1], p[kind == 1] = 1 + i[kind == 1] % 3, i[kind == 1] % 5
    iov = np.zeros(n, V.IOV_DTYPE)
    iov["hdr_len"], iov["payload_len"] = h, p
    iov["hdr_off"] = 5 + np.cumsum(h + i % 3) - (h + i % 3)         # (unused bytes between the slices)
    iov["payload_off"] = 3 + np.cumsum(p + i % 5) - (p + i % 5)
    iov["wire_off"] = 0xDEAD0000 + i                                  # ignored by the call
    lim = None
    if per_record:
        lim = np.array(FIV_LIMITS, np.uint32)[rng.integers(0, len(FIV_LIMITS), n)]
        for at, v in ((R_PLAN - 5, 0), (R_PLAN - 4, 0x80000000), (R_PLAN - 1, 3), (R_PLAN, 3), (R_PLAN + 3, 0),
                      (R_PLAN + 4, 0x80000000)):
            if at < n:
                lim[at] = v
        lim.setflags(write=False)
    iov.setflags(write=False)
    return iov, lim


def fiv_lost_carry(m):
    """fragment_iov_model.fragment_iov's result (nothing cut by a capacity) ->
    what fragiov_blkscan without its carry leaves: dict(out_off, piece_off,
    result, pieces, marks), the last two as the bytes of the buffers, SENT
    where nothing is written. status does not depend on the scan here."""
    n = len(m["status"])
    po = m["piece_off"].astype(np.int64)
    pieces = m["pieces"]
    is_mark = pieces["src"] == V.PIECE_MARK
    nf = np.concatenate(([0], np.cumsum(is_mark)))[po]               # fragments before record i; nf[n]: all
    multi = np.concatenate(([0], np.cumsum(np.diff(nf) > 1)))
    out = {"out_off": drop_carry(m["out_off"], R_PLAN), "piece_off": drop_carry(m["piece_off"], R_PLAN)}
    nf_w, multi_w = drop_carry(nf, R_PLAN), drop_carry(multi, R_PLAN)
    out["result"] = np.array([nf_w[n], out["out_off"][n], multi_w[n], out["piece_off"][n]], np.uint64)
    rec = np.repeat(np.arange(n), np.diff(po))                       # the record of every piece
    start = rec // R_PLAN * R_PLAN                                   # ... and its round's first record
    moved = pieces.copy()
    moved["off"][is_mark] -= (4 * nf[start][is_mark]).astype(np.uint64)
    blank = np.frombuffer(bytes([SENT]) * 16, V.PIECE_DTYPE)
    out["pieces"] = scatter(np.arange(len(pieces)) - po[start], moved, len(pieces), blank).view(np.uint8)
    marks = np.frombuffer(m["marks"], np.uint32)
    frag_rec = np.repeat(np.arange(n), np.diff(nf))
    fstart = frag_rec // R_PLAN * R_PLAN
    out["marks"] = scatter(np.arange(len(marks)) - nf[fstart], marks, len(marks), np.uint32(0xA5A5A5A5)).view(np.uint8)
    return out


# ---------------------------------------------------------------------------
# onc_piece_offsets / onc_gather_pieces
# ---------------------------------------------------------------------------
GATHER_LENS = (64, 300, 1000)
GATHER_BAD = ("none", "late", "both")
# (a first bad piece in round two with more behind it takes three pieces there; bad pieces in two rounds, two rounds)
GATHER_CASES = [(n, bad) for n in PLAN_SIZES for bad in GATHER_BAD
                if bad == "none" or (bad == "late" and n >= R_PLAN + 3) or (bad == "both" and n > R_PLAN)]


@functools.lru_cache(maxsize=None)
def gather_case(n, bad):
    """-> (pieces, sources, the bad pieces' indices): n pieces of 0..3 bytes
    from all three sources. bad = "none"; "late": the first bad piece at an
    index >= R_PLAN, more of them behind it; "both": bad pieces in round one
    and in the later rounds. A bad piece points past its source's end, or names
    source 3: it is never read."""
    rng = np.random.default_rng(9100 + n + GATHER_BAD.index(bad))
    lens = np.array(GATHER_LENS)
    src = rng.integers(0, 3, n)
    ln = rng.integers(0, 4, n)
    off = rng.integers(0, lens[src] - 3)
    if n > R_PLAN:
        ln[R_PLAN] = max(ln[R_PLAN], 1)              # round two's first piece has a byte to put in the wrong place
    where = []
    if bad == "late":
        assert n >= R_PLAN + 3, "a first bad piece in round two with more behind it takes three pieces there"
        first = R_PLAN + (n - R_PLAN) // 3
        where = sorted({first, first + 1, first + (n - first) // 2, n - 1})
    elif bad == "both":
        assert n > R_PLAN
        where = sorted({1000, R_PLAN - 1, R_PLAN, R_PLAN + (n - R_PLAN) // 2, n - 1})
    for j, at in enumerate(where):
        s = int(src[at])
        off[at], ln[at], src[at] = ((lens[s] + 1, 2, s), (5, 1, 3), (lens[s] - 1, 3, s))[j % 3]
    pieces = np.zeros(n, V.PIECE_DTYPE)
    pieces["off"], pieces["len"], pieces["src"] = off, ln, src
    pieces.setflags(write=False)
    srng = np.random.default_rng(9199)
    sources = [srng.integers(0, 256, k, dtype=np.uint8) for k in GATHER_LENS]
    return pieces, sources, where


def gather_lost_carry(pieces, sources, pos, res, where):
    """The model's piece_pos and result -> (piece_pos, result, stream bytes) of
    gath_blkscan without its carry. first_bad is the minimum over the last
    round alone (n: none there); the stream is what onc_gather_pieces writes
    from the wrong positions into SENT bytes."""
    n = len(pieces)
    w_pos = drop_carry(pos, R_PLAN)
    lo = last_round(n, R_PLAN).start
    late = [i for i in where if i >= lo]
    w_res = np.array([w_pos[n], len(late), late[0] if late else n], np.uint64)
    out = np.full(int(res[0]), SENT, np.uint8)
    G.gather(pieces, w_pos, sources, 0, len(out), out)
    return w_pos, w_res, out


# ---------------------------------------------------------------------------
# onc_payload_slots
# ---------------------------------------------------------------------------
PAY_LENS = (0, 1, 15, 16, 17, 4095, 4096, 4097)
PAY_HEAD = 160
INVALID_LENGTH = 10


@functools.lru_cache(maxsize=None)
def payload_case(n):
    """-> (msgs, status): descriptors as tests/test_gpu_payload.py builds them
    for the heads form (head_len PAY_HEAD): OK Calls and accepted-success
    Replies with every length of PAY_LENS, denied and non-success Replies with
    a payload_len, non-OK statuses over non-zero descriptors."""
    rng = np.random.default_rng(9200 + n)
    m = np.zeros(n, L.MSG_DTYPE)
    r = np.arange(n)
    m["xid"] = r + 1000
    # 0, 1: call; 2: success reply; 3: denied; 4: accepted, not success; 5: call, bad status (record R_PLAN, round
    # two's first and in one case its only one: a Call with a payload)
    kind = (r + 2) % 6
    m["msg_type"] = np.where(np.isin(kind, (0, 1, 5)), L.MSG_CALL, L.MSG_REPLY)
    m["reply_stat"] = np.where(kind == 3, L.REPLY_DENIED, L.REPLY_ACCEPTED)
    m["stat"] = np.where(kind == 4, rng.integers(1, 6, n), 0)
    m["payload_len"] = np.array(PAY_LENS)[(r // 6) % len(PAY_LENS)]
    m["f0"], m["f1"], m["f2"] = 100003, 4, rng.integers(0, 20, n)
    m["payload_off"] = r.astype(np.uint64) * PAY_HEAD + rng.integers(28, PAY_HEAD, n).astype(np.uint64)
    m["cred_ref"], m["verf_ref"] = rng.integers(0, 1 << 40, n), rng.integers(0, 1 << 40, n)
    status = np.where(kind == 5, rng.choice((1, INVALID_LENGTH, 106), n), 0).astype(np.int32)
    m.setflags(write=False)
    status.setflags(write=False)
    return m, status


def payload_lost_carry(want):
    """payload_model.payload_slots' result (want_msgs_out) -> dict(slot_off,
    result, msgs_out) of pay_blkscan without its carry. pay_pos and pay_len do
    not depend on the scan."""
    n = len(want["pay_len"])
    has = want["pay_len"] > 0
    k = np.concatenate(([0], np.cumsum(has)))
    nbytes = np.concatenate(([0], np.cumsum(want["pay_len"].astype(np.uint64))))
    slot = drop_carry(want["slot_off"], R_PLAN)
    out = want["msgs_out"].copy()
    out["payload_off"][has] = slot[:n][has]
    return {"slot_off": slot, "msgs_out": out,
            "result": np.array([drop_carry(k, R_PLAN)[n], drop_carry(nbytes, R_PLAN)[n], slot[n]], np.uint64)}


# ---------------------------------------------------------------------------
# onc_route_calls
# ---------------------------------------------------------------------------
ROUTE_SHAPES = ("every", "late", "early")
# (n = R_ROUTE has no record at or behind R_ROUTE: "every" alone)
ROUTE_CASES = [(which, n, shape) for which in ("small", "wide") for n in ROUTE_SIZES for shape in ROUTE_SHAPES
               if n > R_ROUTE or shape == "every"]


@functools.lru_cache(maxsize=None)
def route_table(which):
    """-> (rows, nh, a key per handler, keys no entry serves: PROG_UNAVAIL,
    PROG_MISMATCH, PROC_UNAVAIL). "small": the table of
    test_gpu_route.test_end_to_end_300_records; "wide": 1024 entries over 253
    handlers, which gives 256 bins and the most bin bits."""
    if which == "small":
        rows = [(100003, 3, 0, 4, 0, 0), (100003, 3, 6, 10, 4, 1), (100003, 4, 0, 2, 5, 0), (100005, 3, 0, 6, 6, 1)]
        nh, miss = 7, [(7, 7, 7), (100003, 9, 0), (100003, 3, 4)]
    else:
        nh = 253
        rows = [(100 + i // 4, 1 + (i // 2) % 2, 1000 * (i % 2), 1 + i % 3, i % nh, RM.ONE_HANDLER)
                for i in range(1024)]
        miss = [(7, 7, 7), (100, 9, 0), (100, 1, 500)]
    key_of = {}
    for p, v, pf, pc, hf, fl in rows:
        for c in range(pc):
            key_of.setdefault(hf + (0 if fl & RM.ONE_HANDLER else c), (p, v, pf + c))
    assert sorted(key_of) == list(range(nh))
    return rows, nh, key_of, miss


def route_bins(n, nb, shape, B):
    """The bin of every record. "every": every bin before record R_ROUTE and,
    as far as the records reach, behind it; "late": bin B only at indices >=
    R_ROUTE (record R_ROUTE itself and every other one behind it); "early":
    bin B only below R_ROUTE."""
    rng = np.random.default_rng(9300 + n % 9973 + 7 * nb + ROUTE_SHAPES.index(shape))
    bins = rng.integers(0, nb, n)
    R = R_ROUTE
    if shape == "every":
        bins[:nb] = np.arange(nb)
        k = min(nb, max(n - R, 0))
        bins[R:R + k] = (np.arange(k) + 5) % nb
    elif shape == "late":
        assert n > R
        head = bins[:R]
        head[head == B] = B + 1
        bins[R::2] = B
    else:
        tail = bins[R:]
        tail[tail == B] = B + 1
        bins[5] = B
    return bins


def route_case(n, which, shape):
    """-> (msgs, status, table, nh, bins, B): descriptors and statuses that the
    model sends to `bins` — handler bins through the table's keys, rejected
    Calls of all three kinds, not-a-Call as msg_type 1 and 7, failed records as
    random bytes — in the style of test_gpu_route.records_for. B: the bin the
    shape is about (a handler in the middle)."""
    rows, nh, key_of, miss = route_table(which)
    B = nh // 2
    bins = route_bins(n, nh + 3, shape, B)
    rng = np.random.default_rng(9400 + n % 9973 + nh)
    m = np.zeros(n, L.MSG_DTYPE)
    r = np.arange(n)
    m["xid"] = rng.integers(0, 1 << 32, n)
    m["payload_len"], m["payload_off"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 63, n)
    m["cred_ref"], m["verf_kind_len"] = rng.integers(0, 1 << 40, n), rng.integers(0, 1 << 32, n)
    keys = np.array([key_of[h] for h in range(nh)] + miss, np.uint32)
    at = np.where(bins < nh, bins, nh + r % 3)
    call = bins <= nh
    for j, f in enumerate(("f0", "f1", "f2")):
        m[f][call] = keys[at[call], j]
    m["msg_type"][bins == nh + 1] = np.where(r[bins == nh + 1] % 2 == 0, L.MSG_REPLY, 7)
    failed = bins == nh + 2
    m[failed] = np.frombuffer(rng.bytes(64 * int(failed.sum())), L.MSG_DTYPE)
    status = np.zeros(n, np.int32)
    status[failed] = np.array((1, 10, 106, -3), np.int32)[r[failed] % 4]
    for a in (m, status, bins):
        a.setflags(write=False)
    return m, status, RM.table(rows), nh, bins, B


def route_lost_carry(msgs, want, nh):
    """route_model's result -> dict(order, bin_first, result, calls_out,
    replies) of route_scan_bins without its carry; the descriptor arrays as
    bytes, SENT where no record lands. route[] does not depend on the scan."""
    n = len(msgs)
    dest, first = partition_without_carry(want["route"], nh + 3, R_ROUTE)
    cnt = np.diff(first)
    by_rec = np.empty(n, L.MSG_DTYPE)
    by_rec[want["order"]] = want["replies"]
    blank = np.frombuffer(bytes([SENT]) * 64, L.MSG_DTYPE)
    return {"order": scatter(dest, np.arange(n, dtype=np.uint32), n, np.uint32(U32)),
            "bin_first": first.astype(np.uint64),
            "result": np.array([first[nh], cnt[nh], cnt[nh + 1] + cnt[nh + 2], 0], np.uint64),
            "calls_out": scatter(dest, msgs, n, blank).view(np.uint8),
            "replies": scatter(dest, by_rec, n, blank).view(np.uint8)}


# ---------------------------------------------------------------------------
# onc_group_by_conn
# ---------------------------------------------------------------------------
GROUP_NCONNS = (200, 70000)          # one radix pass, and three
GROUP_CASES = [(n, nconn, via) for n in GROUP_SIZES for nconn in GROUP_NCONNS for via in (False, True)]


def conns_for(n, nconn, seed):
    """Connections over the whole range, a few of them busy, some items dropped
    (test_gpu_group.conns_for)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, nconn + 1, n).astype(np.uint32)                 # (nconn itself: dropped)
    busy = rng.integers(0, nconn + 1, 5).astype(np.uint32)
    pick = rng.random(n) < 0.4
    c[pick] = busy[rng.integers(0, 5, n)][pick]
    c[rng.random(n) < 0.05] = U32
    return c


def group_case(n, nconn, with_via):
    """-> (rec_conn, via or None): with_via, the items are a permutation's
    first n entries of a rec_conn nine longer."""
    if not with_via:
        rc, via = conns_for(n, nconn, 9500 + nconn), None
    else:
        rc = conns_for(n + 9, nconn, 9501 + nconn)
        via = np.random.default_rng(9502 + n % 9973).permutation(n + 9)[:n].astype(np.uint32)
        via.setflags(write=False)
    rc.setflags(write=False)
    return rc, via


def group_lost_carry(key, nconn, msgs):
    """The items' clamped keys -> dict(order, conn_first, result, msgs_out) of
    a sort whose every pass runs group_scan_digits without its carry. A slot no
    item lands in keeps key 0, index 0; conn_first is group_bounds' 32-step
    lower bound over whatever keys the last pass left."""
    n = len(key)
    k, idx = np.asarray(key, np.int64), np.arange(n, dtype=np.int64)
    for p in range(GM.passes(nconn)):
        dest, _ = partition_without_carry((k >> (8 * p)) & 255, 256, R_GROUP)
        k, idx = scatter(dest, k, n, np.int64(0)), scatter(dest, idx, n, np.int64(0))
    c = np.arange(nconn + 2, dtype=np.int64)
    lo, hi = np.zeros(nconn + 2, np.int64), np.full(nconn + 2, n, np.int64)
    for _ in range(32):                                                  # group_plan.h group_lower_bound
        go = lo < hi
        mid = lo + (hi - lo) // 2
        below = go & (k[np.minimum(mid, n - 1)] < c)
        lo = np.where(below, mid + 1, lo)
        hi = np.where(go & ~below, mid, hi)
    sent = int(lo[nconn])
    return {"order": idx.astype(np.uint32), "conn_first": lo.astype(np.uint64),
            "result": np.array([sent, n - sent, np.count_nonzero(np.diff(lo[:nconn + 1]) > 0)], np.uint64),
            "msgs_out": np.asarray(msgs)[idx]}


def descriptors(n, seed=0):
    """n descriptors of random bytes whose payload_off lies above 2^32
    (test_gpu_group.descriptors)."""
    rng = np.random.default_rng(1000 + seed)
    m = np.frombuffer(rng.integers(0, 256, 64 * n, dtype=np.uint8).tobytes(), L.MSG_DTYPE).copy()
    m["payload_off"] = (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(0x100000001)
    return m


# ---------------------------------------------------------------------------
# onc_match_replies
# ---------------------------------------------------------------------------
MATCH_N = 3 * TILE + 1
# (np, the last entry answered, tag_out and still asked for)
MATCH_PENDING = [(R_MATCH + 1, False, True), (R_MATCH + 1, True, True), (R_MATCH + 1, False, False),
                 (2 * R_MATCH + 1, False, True), (2 * R_MATCH + 1, True, True)]


def distinct_keys(count, seed):
    """`count` different (conn, xid) keys: xids counting up from a random start
    on five connections (test_gpu_match.distinct_keys)."""
    rng = np.random.default_rng(seed + 2000)
    conn = rng.integers(0, 1 << 32, 5, dtype=np.uint64)
    x0 = int(rng.integers(0, 1 << 31))
    i = np.arange(count, dtype=np.uint64)
    return np.stack([conn[i % 5], (np.uint64(x0) + i // 5) & np.uint64(U32)], axis=1)


def _pending(keys, seed):
    p = np.zeros(len(keys), L.PENDING_DTYPE)
    p["conn"], p["xid"] = keys[:, 0].astype(np.uint32), keys[:, 1].astype(np.uint32)
    p["tag"] = np.random.default_rng(seed).integers(0, 1 << 64, len(keys), dtype=np.uint64)
    return p


def _replies(keys, seed):
    """OK Reply descriptors for the keys, every word the call does not look at
    random -> (msgs, status, rec_conn)."""
    n = len(keys)
    m = np.frombuffer(np.random.default_rng(seed).bytes(64 * n), L.MSG_DTYPE).copy()
    m["xid"] = keys[:, 1].astype(np.uint32)
    m["msg_type"] = L.MSG_REPLY
    return m, np.zeros(n, np.int32), keys[:, 0].astype(np.uint32)


def match_pending_case(npend, answer_last):
    """The pending side: npend = R_MATCH + 1 or 2 R_MATCH + 1 distinct entries
    and MATCH_N records -> (msgs, status, rec_conn, pending, answered). The
    Replies answer 1500 entries of the first three tiles, 600 of the tiles from
    1024 on (as far as the list has more than one entry there) and, for 2
    R_MATCH + 1, 300 of the last tiles of round two; the rest of the batch are
    a few duplicates, unknown keys, records that are no Replies and failed
    ones. The last entry — a round's only one — is answered or not as asked:
    unanswered, its place in `still` is the carry; answered, the Reply hits a
    tile of the last round."""
    rng = np.random.default_rng(9600 + npend % 9973 + (1 if answer_last else 0))
    keys = distinct_keys(npend, 61)
    pick = [rng.choice(3 * TILE, 1500, replace=False)]
    if npend > R_MATCH + 1:
        pick.append(R_MATCH + rng.choice(R_MATCH - 2 * TILE, 600, replace=False))
        pick.append(2 * R_MATCH - 2 * TILE + rng.choice(2 * TILE, 300, replace=False))
    if answer_last:
        pick.append(np.array([npend - 1]))
    answered = np.concatenate(pick)
    other = distinct_keys(MATCH_N, 62)                                  # (another start: not pending)
    rk = np.concatenate([keys[answered], keys[answered[:40]], other])[:MATCH_N]
    cls = np.zeros(MATCH_N, int)
    extra = np.arange(len(answered) + 40, MATCH_N)
    cls[extra[1::3]], cls[extra[2::3]] = 3, 4                           # no Reply; failed
    o = rng.permutation(MATCH_N)
    m, status, rc = _replies(rk[o], 63)
    cls = cls[o]
    m["msg_type"][cls == 3] = np.where(np.arange(MATCH_N)[cls == 3] % 2 == 0, L.MSG_CALL, 7)
    status[cls == 4] = 106
    return m, status, rc, _pending(keys, 64), np.sort(answered)


MATCH_REC_N, MATCH_REC_NP = R_MATCH + 1000, 5000


def match_record_case():
    """The record side: MATCH_REC_N records against MATCH_REC_NP entries -> (msgs,
    status, rec_conn, pending). Entries 0 .. 2999 are answered by records
    anywhere (first below R_MATCH: the later ones are duplicates), 4000 .. 4999
    only by records >= R_MATCH (matched and duplicates there), 3000 .. 3999 by
    none; unknown keys, records that are no Replies and failed ones everywhere.
    So each of the five classes has records on both sides of R_MATCH, and in
    the first tile."""
    rng = np.random.default_rng(9700)
    n = MATCH_REC_N
    keys = distinct_keys(MATCH_REC_NP, 71)
    other = distinct_keys(4096, 72)
    r = np.arange(n)
    cls = rng.choice(4, n, p=(0.2, 0.3, 0.25, 0.25))                    # a pending key, unknown, no Reply, failed
    p = rng.integers(0, 3000, n)
    late = r >= R_MATCH
    p[late] = np.where(rng.random(int(late.sum())) < 0.8, rng.integers(4000, 5000, int(late.sum())), p[late])
    cls[late] = rng.choice(4, int(late.sum()), p=(0.55, 0.15, 0.15, 0.15))
    rk = np.where((cls == 1)[:, None], other[r % len(other)], keys[p])
    m, status, rc = _replies(rk, 73)
    m["msg_type"][cls == 2] = np.where(r[cls == 2] % 2 == 0, L.MSG_CALL, 7)
    status[cls == 3] = 106
    return m, status, rc, _pending(keys, 74)


def match_lost_carry(pend, want, n):
    """match_model's result -> dict(still, result) of match_scan without its
    carries: an unanswered entry of pending round k lands short of the
    unanswered entries of the rounds before k (still: all npend slots as bytes,
    SENT where no entry lands) and result[5] is the last round's count alone;
    a class sum keeps, of every thread's stride over the record tiles, the last
    tile alone. match, hit and tag_out do not depend on the scan."""
    npend = len(pend)
    waiting = want["hit"] == U32
    before = np.concatenate(([0], np.cumsum(waiting)))
    w_before = drop_carry(before, R_MATCH)
    dest = np.where(waiting, w_before[:npend], -1)
    blank = np.frombuffer(bytes([SENT]) * 16, L.PENDING_DTYPE)
    still = scatter(dest, pend, npend, blank).view(np.uint8)
    rtiles = (n + TILE - 1) // TILE
    t = np.arange(n) // TILE
    kept = t + TILE >= rtiles                                 # the tile is the last one of its thread's stride
    m = want["match"][kept]
    res = [int((m < 0xFFFFFFFC).sum())]
    res += [int((m == v).sum()) for v in (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC)]
    return {"still": still, "result": np.array(res + [w_before[npend]], np.uint64)}
