"""Host model of the zero-copy receive of fragmented records:
onc_defragment_heads (only each record's head is reassembled, into a
fixed-stride slot) and onc_decode_heads (records of which only the head is
present), for tests/test_heads_model.py on the CPU and tests/test_gpu_heads.py
on the GPU.

Not a test file and not product code. The gather model is derived from
fragment_streams_model.defragment_extents — a slot is the prefix of the packed
record — and serial_heads is the loop of include/onc_rpc.h written out on its
own; the decode model starts from the oracle's decode of the whole packed
records. Expected values come from here, never from the code under test.
"""
from __future__ import annotations

import struct

import numpy as np

import fragment_model as FR
import fragment_streams_model as FS
import onc_rpc_amd.layout as L

OK = 0
ENC_TOO_LONG, ENC_WRITE_ZERO = FR.ENC_TOO_LONG, FR.ENC_WRITE_ZERO
DEC_BAD_EXTENT, EXTENT_HEAD_SHORT = 106, 4
HEAD_SPAN_MAX = 724                 # include/onc_rpc.h ONC_HEAD_SPAN_MAX
HEAD_FULL = 736                     # ... rounded up to 16: every header fits
HEAD_SHORT = (DEC_BAD_EXTENT, EXTENT_HEAD_SHORT, 0)
_BE = struct.Struct(">I")


def head_len_ok(h):
    return 64 <= h <= 4096 and h % 16 == 0


# ---------------------------------------------------------------------------
# onc_defragment_heads
# ---------------------------------------------------------------------------
def defragment_heads(wire, frag_start, frag_len, head_len, max_records=None):
    """From the packed form: dict(slots: per record the bytes its slot
    receives (None: nothing is written), rec_len u32[n], rec_frag u64[n + 1],
    frag_pre u64[nfrag], status i32[n], result u64[6]); max_records None: a
    slot for every record."""
    assert head_len_ok(head_len)
    m = FS.defragment_extents(wire, frag_start, frag_len)
    n, nfrag = len(m["status"]), len(frag_start)
    cap = n if max_records is None else max_records
    rec_len = np.diff(m["rec_off"].astype(np.int64)).astype(np.uint32)      # 0 for a record that is too long
    status, slots = [], []
    for r in range(n):
        if m["status"][r] == ENC_TOO_LONG:
            status.append(ENC_TOO_LONG)
            slots.append(None)
        elif r < cap:
            status.append(OK)
            slots.append(m["records"][r][:head_len])
        else:
            status.append(ENC_WRITE_ZERO)
            slots.append(None)
    # which fragments a record is, and the body bytes before each of them
    wire = bytes(wire)
    last = np.array([wire[int(a)] >> 7 for a in frag_start], bool)
    ends = np.nonzero(last)[0]
    rec_frag = np.concatenate(([0], ends + 1)).astype(np.uint64)
    body = np.asarray(frag_len, np.int64) - 4
    frag_pre = np.zeros(nfrag, np.uint64)
    for j in range(nfrag):
        first = int(rec_frag[np.searchsorted(rec_frag, j, side="right") - 1])
        frag_pre[j] = int(body[first:j].sum())
    res = m["result"]
    result = np.array([n, res[1], n * head_len, res[3], res[4], res[5]], np.uint64)
    return {"slots": slots, "rec_len": rec_len, "rec_frag": rec_frag, "frag_pre": frag_pre,
            "status": np.array(status, np.int32), "result": result}


def serial_heads(wire, frag_start, frag_len, head_len, max_records):
    """The loop of include/onc_rpc.h, line by line. Same dict as defragment_heads."""
    wire = bytes(wire)
    nfrag = len(frag_start)
    rec_len, rec_frag, frag_pre, status, slots = [], [], [], [], []
    r = first = B = multi = 0
    bodies = []
    for j in range(nfrag):
        s, ln = int(frag_start[j]), int(frag_len[j])
        frag_pre.append(B)
        B += ln - 4
        bodies.append(wire[s + 4:s + ln])
        if wire[s] & 0x80:
            rec_frag.append(first)
            if B >= 1 << 31:
                rec_len.append(0)
                status.append(ENC_TOO_LONG)
                slots.append(None)
            else:
                rec_len.append(4 + B)
                ok = r < max_records
                status.append(OK if ok else ENC_WRITE_ZERO)
                slot = None
                if ok:
                    slot = (_BE.pack(0x80000000 | B) + b"".join(bodies))[:min(4 + B, head_len)]
                slots.append(slot)
            multi += j > first
            r += 1
            first = j + 1
            B = 0
            bodies = []
    rec_frag.append(first)
    return {"slots": slots, "rec_len": np.array(rec_len, np.uint32), "rec_frag": np.array(rec_frag, np.uint64),
            "frag_pre": np.array(frag_pre, np.uint64), "status": np.array(status, np.int32),
            "result": np.array([r, first, r * head_len, nfrag - first, B, multi], np.uint64)}


def same_heads(a, b):
    return [k for k in ("rec_len", "rec_frag", "frag_pre", "status", "result") if not np.array_equal(a[k], b[k])] + \
        (["slots"] if a["slots"] != b["slots"] else [])


def expected_heads(model, head_len, size, sentinel):
    """The `size` bytes from `heads` on after the call: OK records' heads in
    their slots, the sentinel everywhere else."""
    a = np.full(size, sentinel, np.uint8)
    for r, slot in enumerate(model["slots"]):
        if slot is not None:
            a[r * head_len:r * head_len + len(slot)] = np.frombuffer(slot, np.uint8)
    return a


def locate(model, frag_start, r, p):
    """The wire offset of record byte p >= 4 of record r, through rec_frag and
    frag_pre as the header says."""
    lo, hi = int(model["rec_frag"][r]), int(model["rec_frag"][r + 1])
    pre = model["frag_pre"][lo:hi].astype(np.int64)
    j = lo + int(np.searchsorted(pre, p - 4, side="right")) - 1
    return int(frag_start[j]) + 4 + (p - 4 - int(model["frag_pre"][j]))


def gather(model, wire, frag_start, frag_len, r, pos, length):
    """Record bytes [pos, pos + length) of record r, gathered from the wire
    fragment by fragment (pos >= 4)."""
    wire = bytes(wire)
    out = []
    lo, hi = int(model["rec_frag"][r]), int(model["rec_frag"][r + 1])
    x, left = pos - 4, length
    for j in range(lo, hi):
        body = int(frag_len[j]) - 4
        at = x - int(model["frag_pre"][j])
        if left == 0 or at < 0 or at >= body:
            continue
        take = min(left, body - at)
        s = int(frag_start[j]) + 4 + at
        out.append(wire[s:s + take])
        x += take
        left -= take
    assert left == 0
    return b"".join(out)


GATHER_GROUP = 256                  # defrag_heads.hip kDhThreads: chunks per step of one workgroup


def stride_steps_stream(nrec=20, head_len=HEAD_FULL, seed=89):
    """-> (wire, frag_start, frag_len, too_long): `nrec` records whose slots
    are nrec * head_len / 16 chunks — with 20 at 736 that is 920, four steps
    of heads_gather's stride loop in one workgroup. By turns a record is one
    fragment longer than its slot, fragments of 1..40 bytes with empty ones
    among them (a seam in almost every chunk), shorter than its slot, and
    empty. Record `too_long` (slots of the third step) is two fragments whose
    lengths say 2^30 body bytes each: B = 2^31, ONC_ENC_TOO_LONG. The wire
    holds only their marks — of a fragment the plan reads the first byte, and
    of a record that is too long the gather reads nothing — so the model for
    this stream is serial_heads, which takes B from frag_len as the plan does."""
    rng = np.random.default_rng(seed)
    too_long = (2 * GATHER_GROUP + 40) * 16 // head_len
    parts, start, length, pos = [], [], [], 0

    def put(mark, body, declared=None):
        nonlocal pos
        parts.append(_BE.pack(mark) + body)
        start.append(pos)
        length.append(4 + len(body) if declared is None else declared)
        pos += 4 + len(body)

    for r in range(nrec):
        if r == too_long:
            put(1 << 30, b"", declared=4 + (1 << 30))
            put(FR.LAST | (1 << 30), b"", declared=4 + (1 << 30))
            continue
        which = r % 4
        if which == 0:
            lens = [head_len + 100 + r]
        elif which == 1:
            lens = rng.choice((0, 1, 2, 3, 5, 17, 40), 120).tolist()
        elif which == 2:
            lens = [100, 0, 0, head_len // 2 - 133 + r]
        else:
            lens = [0] if r % 8 == 3 else [0, 0, 9, 0]
        for i, n in enumerate(lens):
            put((FR.LAST if i == len(lens) - 1 else 0) | n, rng.bytes(n))
    return b"".join(parts), np.array(start, np.uint64), np.array(length, np.uint32), too_long


# ---------------------------------------------------------------------------
# onc_decode_heads
# ---------------------------------------------------------------------------
def heads_of(records, head_len, fill=0):
    """(heads bytes, rec_len): every record's first head_len bytes in its slot,
    `fill` in the rest of the slot."""
    buf = np.full(max(len(records), 1) * head_len, fill, np.uint8)
    for i, rec in enumerate(records):
        p = min(len(rec), head_len)
        buf[i * head_len:i * head_len + p] = np.frombuffer(rec[:p], np.uint8)
    return buf[:len(records) * head_len].tobytes(), np.array([len(r) for r in records], np.uint32)


def has_payload(m):
    return (m["msg_type"] == L.MSG_CALL) | ((m["msg_type"] == L.MSG_REPLY) & (m["reply_stat"] == L.REPLY_ACCEPTED) &
                                            (m["stat"] == 0))


def decode_heads(oracle, records, head_len, mode):
    """The expected onc_decode_heads of whole records `records` (a list of
    byte strings) presented through heads of head_len bytes -> (msgs, unix,
    status, aux0, aux1, either): the oracle's decode of the packed records
    with every offset rebased to i * head_len, ONC_EXTENT_HEAD_SHORT by rule
    (b) for the records the oracle decodes OK, and the AUTH_UNIX slots ranked
    again per 64 records. either[i]: the oracle rejects record i and the record
    is longer than its head — the outcome is the oracle's error or HEAD_SHORT
    (the model cannot tell which read comes first); a test states it itself."""
    n = len(records)
    lens = np.array([len(r) for r in records], np.int64)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    wire = np.frombuffer(b"".join(records) + b"\0" * 16, np.uint8).copy()
    om, ou, ost, oa0, oa1 = oracle.decode_batch(wire, off, mode)
    msgs = om.copy()
    status, aux0, aux1 = ost.copy(), oa0.copy(), oa1.copy()
    unix = np.zeros(max(2 * n, 1), L.UNIX_DTYPE)
    P = np.minimum(lens, head_len)
    pay = has_payload(om)
    either = (ost != OK) & (lens > head_len)
    for i in range(n):
        if ost[i] != OK:
            continue
        hdr_end = int(om["payload_off"][i]) - int(off[i]) if pay[i] else int(lens[i])
        if hdr_end > P[i]:
            status[i], aux0[i], aux1[i] = HEAD_SHORT
            msgs[i] = np.zeros(1, L.MSG_DTYPE)[0]
    cred_u, verf_u = L.unix_used(om, status)
    for g0 in range(0, n, 64):
        rank = 2 * g0
        for i in range(g0, min(g0 + 64, n)):
            if status[i] != OK:
                continue
            d = i * head_len - int(off[i])
            if pay[i]:
                msgs["payload_off"][i] = int(om["payload_off"][i]) + d
            call = om["msg_type"][i] == L.MSG_CALL
            parsed = {"cred": call, "verf": call or om["reply_stat"][i] == L.REPLY_ACCEPTED}
            for f, used in (("cred", cred_u[i]), ("verf", verf_u[i])):
                if used:
                    row = ou[int(om[f + "_ref"][i])].copy()
                    row["name_off"] = int(row["name_off"]) + d
                    unix[rank] = row
                    msgs[f + "_ref"][i] = rank
                    rank += 1
                elif parsed[f]:
                    msgs[f + "_ref"][i] = int(om[f + "_ref"][i]) + d
    return msgs, unix[:2 * n], status, aux0, aux1, either


def check_decode(got, want, what="", exact=None):
    """onc_decode_heads' outputs == the model's: statuses and aux words
    (either-or records: the oracle's error or HEAD_SHORT, unless `exact` maps
    the record to its (status, aux0, aux1)), descriptors byte for byte, the
    AUTH_UNIX slots of OK records."""
    gm, gu, gs, ga0, ga1 = got
    wm, wu, ws, wa0, wa1, either = want
    exact = exact or {}
    for i in range(len(ws)):
        g = (int(gs[i]), int(ga0[i]), int(ga1[i]))
        w = (int(ws[i]), int(wa0[i]), int(wa1[i]))
        if i in exact:
            assert g == tuple(exact[i]), f"{what}: record {i}: {g} != stated {exact[i]}"
        elif either[i]:
            assert g in (w, HEAD_SHORT), f"{what}: record {i}: {g} is neither {w} nor HEAD_SHORT"
        else:
            assert g == w, f"{what}: record {i}: {g} != {w}"
    gb, wb = gm.view(np.uint8).reshape(-1, 64), wm.view(np.uint8).reshape(-1, 64)
    bad = np.nonzero((gb != wb).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: descriptor mismatch at {bad[:10]}: {gm[bad[0]]} vs {wm[bad[0]]}"
    cred, verf = L.unix_used(wm, ws)
    idx = np.sort(np.concatenate([wm["cred_ref"][cred], wm["verf_ref"][verf]]).astype(np.int64))
    if len(idx):
        gu8, wu8 = gu.view(np.uint8).reshape(-1, 96)[idx], wu.view(np.uint8).reshape(-1, 96)[idx]
        bad = np.nonzero((gu8 != wu8).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: unix slot mismatch at {idx[bad[:10]]}"


# ---------------------------------------------------------------------------
# records the tests build
# ---------------------------------------------------------------------------
def be(*words):
    return b"".join(_BE.pack(w & 0xFFFFFFFF) for w in words)


def opaque(body):
    return be(len(body)) + body + b"\0" * (-len(body) % 4)


def auth(flavor, body):
    return be(flavor) + opaque(body)


def unix_body(stamp, name, uid, gid, gids):
    return be(stamp) + opaque(name) + be(uid, gid, len(gids), *gids)


def record(body):
    return be(0x80000000 | len(body)) + body


def call(xid, cred, verf, payload, prog=100003, vers=4, proc=1, rpcvers=2):
    return record(be(xid, 0, rpcvers, prog, vers, proc) + cred + verf + payload)


def accepted(xid, verf, stat, rest=b""):
    return record(be(xid, 1, 0) + verf + be(stat) + rest)


AUTH_NONE, AUTH_UNIX, AUTH_SHORT = 0, 1, 2
NONE = auth(AUTH_NONE, b"")


def big_unix_call(xid, payload=b"", name_len=116, ngids=16):
    """An AUTH_UNIX Call with `ngids` gids and a name of name_len bytes ->
    (record, header end S). 16 gids and a 116-byte name make a 200-byte
    credential body, the longest the reference accepts (flavor.rs:83: a longer
    declared length is InvalidLength before the body is parsed)."""
    rng = np.random.default_rng(xid)
    name = bytes(rng.integers(97, 123, name_len, dtype=np.uint8))
    body = unix_body(7, name, 501, 20, list(range(100, 100 + ngids)))
    rec = call(xid, auth(AUTH_UNIX, body), NONE, payload)
    return rec, len(rec) - len(payload)
