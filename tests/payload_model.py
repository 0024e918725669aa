"""Host model of onc_payload_slots / onc_place_payloads (decoded payloads
placed in aligned slots on the device), for tests/test_payload_model.py on the
CPU and tests/test_gpu_payload.py on the GPU.

Not a test file and not product code. Both functions are the loops of
include/onc_rpc.h written out line by line, over numpy arrays. Expected values
come from here, never from the code under test.
"""
from __future__ import annotations

import numpy as np

import onc_rpc_amd.layout as L

OK = 0
ALIGN_MAX = 1 << 20
U32, U64 = (1 << 32) - 1, (1 << 64) - 1


def align_ok(align):
    return 1 <= align <= ALIGN_MAX and align & (align - 1) == 0


def round_up(length, align):
    return (int(length) + align - 1) // align * align


def has_payload(m, status):
    """The `has` of the header's loop for one descriptor."""
    if int(status) != OK or int(m["payload_len"]) == 0:
        return False
    if int(m["msg_type"]) == L.MSG_CALL:
        return True
    return int(m["msg_type"]) == L.MSG_REPLY and int(m["reply_stat"]) == L.REPLY_ACCEPTED and int(m["stat"]) == 0


def payload_slots(msgs, status, align, head_len=0, rec_start=None, want_msgs_out=False):
    """dict(pay_pos u32[n], pay_len u32[n], slot_off u64[n + 1], result u64[3],
    msgs_out (a copy of msgs with payload_off rebased) or None)."""
    assert align_ok(align)
    n = len(msgs)
    pay_pos, pay_len = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    slot_off = np.zeros(n + 1, np.uint64)
    out = np.array(msgs, L.MSG_DTYPE, copy=True) if want_msgs_out else None
    off = k = nbytes = 0
    for r in range(n):
        m = msgs[r]
        has = has_payload(m, status[r])
        base = int(rec_start[r]) if rec_start is not None else r * head_len
        pay_pos[r] = ((int(m["payload_off"]) - base) & U32) if has else 0
        pay_len[r] = int(m["payload_len"]) if has else 0
        slot_off[r] = off
        if out is not None and has:
            out["payload_off"][r] = off
        off += round_up(pay_len[r], align)
        k += has
        nbytes += int(pay_len[r])
    slot_off[n] = off
    return {"pay_pos": pay_pos, "pay_len": pay_len, "slot_off": slot_off,
            "result": np.array([k, nbytes, off], np.uint64), "msgs_out": out}


def slice_ok(pay_pos, pay_len, rec_len, slot_off, dst_cap):
    """The `ok` of the header's loop; no sum is formed (Python's would not
    wrap, the device's would)."""
    pay_pos, pay_len, rec_len, slot_off = int(pay_pos), int(pay_len), int(rec_len), int(slot_off)
    return (pay_pos >= 4 and pay_pos <= rec_len and pay_len <= rec_len - pay_pos and
            slot_off <= dst_cap and pay_len <= dst_cap - slot_off)


def frag_of(frag_pre, lo, hi, x):
    """heads_frag_of: the last j in [lo, hi) with frag_pre[j] <= x
    (frag_pre[lo] == 0 <= x, and frag_pre is sorted within a record)."""
    return lo + int(np.searchsorted(frag_pre[lo:hi], x, side="right")) - 1


def place_payloads(wire, frag_start, frag_len, rec_frag, frag_pre, rec_len, pay_pos, pay_len, slot_off, dst):
    """The copy, into the numpy array `dst` (dst_cap = its length) in place;
    returns the records that were copied. rec_frag = frag_pre = None: the
    identity form."""
    assert (rec_frag is None) == (frag_pre is None)
    wire = np.frombuffer(bytes(wire), np.uint8)
    dst_cap = len(dst)
    done = []
    for r in range(len(pay_len)):
        ln = int(pay_len[r])
        if ln == 0:
            continue
        if not slice_ok(pay_pos[r], ln, rec_len[r], slot_off[r], dst_cap):
            continue
        so = int(slot_off[r])
        for i in range(ln):
            x = int(pay_pos[r]) - 4 + i
            if rec_frag is not None:
                j = frag_of(frag_pre, int(rec_frag[r]), int(rec_frag[r + 1]), x)
                pre = int(frag_pre[j])
            else:
                j, pre = r, 0
            dst[so + i] = wire[int(frag_start[j]) + 4 + (x - pre)]
        done.append(r)
    return done


def place_payloads_fast(wire, frag_start, frag_len, rec_frag, frag_pre, rec_len, pay_pos, pay_len, slot_off, dst):
    """The same result fragment by fragment instead of byte by byte (for the
    long records of the GPU tests); checked against place_payloads in
    tests/test_payload_model.py."""
    assert (rec_frag is None) == (frag_pre is None)
    wire = np.frombuffer(bytes(wire), np.uint8)
    dst_cap = len(dst)
    done = []
    for r in range(len(pay_len)):
        ln = int(pay_len[r])
        if ln == 0 or not slice_ok(pay_pos[r], ln, rec_len[r], slot_off[r], dst_cap):
            continue
        so, x0 = int(slot_off[r]), int(pay_pos[r]) - 4
        if rec_frag is None:
            s = int(frag_start[r]) + 4 + x0
            dst[so:so + ln] = wire[s:s + ln]
        else:
            for j in range(int(rec_frag[r]), int(rec_frag[r + 1])):
                pre, body = int(frag_pre[j]), int(frag_len[j]) - 4
                a, b = max(pre, x0), min(pre + body, x0 + ln)
                if a < b:
                    s = int(frag_start[j]) + 4 + (a - pre)
                    dst[so + a - x0:so + b - x0] = wire[s:s + b - a]
        done.append(r)
    return done


# ---------------------------------------------------------------------------
# streams and slices the tests build
# ---------------------------------------------------------------------------
TILE = 8192          # payload.hip kPlTile: dst bytes per wave and step
STAGE = 128          # payload.hip kPlStage: records of a tile kept in LDS
BODIES = (0, 1, 2, 3, 5, 40)
EMPTY_RUN = 200      # records with pay_len == 0 between two records with payloads


def _mixed_record(rng, nfrag):
    import fragment_model as FR
    lens = rng.choice(BODIES, nfrag)
    return FR.fragment(rng.bytes(int(lens.sum())), np.cumsum(lens)[:-1].tolist())


def place_stream(seed=61, small=False):
    """-> (fragment stream, names): about 700 fragments in about 150 records
    with bodies of 0, 1, 2, 3, 5 and 40 bytes mixed, and behind them
    names["ones"]: a record of 1-byte fragments longer than a tile plus the
    staging, names["long"]: a record whose whole body is longer than four
    tiles, in fragments of 1..3000 bytes with empty ones among them, and
    names["run"]: the first of EMPTY_RUN small records whose slices the tests
    make empty, between two records that keep theirs. small: the same shapes
    cut down for the byte-by-byte model."""
    import fragment_model as FR
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(30 if small else 150):
        recs.append(_mixed_record(rng, 40 if i % 35 == 7 else int(rng.integers(1, 7))))
    names = {}
    names["ones"] = len(recs)
    n1 = 300 if small else TILE + STAGE + 70
    recs.append(b"".join(FR._BE.pack((FR.LAST if i == n1 - 1 else 0) | 1) + rng.bytes(1) for i in range(n1)))
    recs.append(_mixed_record(rng, 5))
    names["long"] = len(recs)
    body = rng.bytes(3000 if small else 4 * TILE + 5000)
    cuts = np.sort(rng.integers(0, len(body) + 1, 6 if small else 30)).tolist()
    recs.append(FR.fragment(body, cuts + cuts[3:5]))            # (equal cuts: empty fragments in the middle)
    names["run"] = len(recs) + 1
    names["run_len"] = 20 if small else EMPTY_RUN
    for i in range(names["run_len"] + 2):
        whole = i % 9 == 0 or i == names["run_len"] + 1      # (both neighbours of the run have 45 body bytes)
        recs.append(FR.fragment(rng.bytes(45), [20]) if whole else _mixed_record(rng, int(rng.integers(1, 4))))
    for i in range(10):
        recs.append(_mixed_record(rng, int(rng.integers(1, 7))))
    return b"".join(recs), names


def tile_run_records(kind, ntiles, origin, fragmented, seed=83):
    """tile_walk_model.layout(kind, ntiles, origin) as records whose payload
    slices, packed at align 1, are the entries (an entry of no output: a
    record without a payload). -> dict(wire, frag_start, frag_len, rec_frag,
    frag_pre, rec_len, pay_pos, pay_len); fragmented: every record cut into 1
    to 5 fragments, an empty one among them now and then; else the identity
    form (rec_frag = frag_pre = None). The positions of the walk are 0, the
    slots and 2^64 - 1."""
    import fragment_model as FR
    import tile_walk_model as TW
    entries, _ = TW.layout(kind, ntiles, origin)
    rng = np.random.default_rng(seed + ntiles)
    parts, rec_frag, frag_pre, rec_len, pay_pos, pay_len = [], [0], [], [], [], []
    for i, (ln, _) in enumerate(entries):
        pre = int(rng.integers(0, 41))
        body = rng.bytes(pre + ln + int(rng.integers(0, 9)))
        cuts = []
        if fragmented and len(body):
            cuts = sorted(rng.integers(0, len(body) + 1, int(rng.integers(0, 4))).tolist())
            if cuts and i % 3 == 0:
                cuts.insert(0, cuts[0])
        parts.append(FR.fragment(body, cuts))
        edges = [0] + cuts
        frag_pre += edges
        rec_frag.append(rec_frag[-1] + len(edges))
        rec_len.append(4 + len(body))
        pay_pos.append(4 + pre if ln else int(rng.integers(0, 50)))
        pay_len.append(ln)
    wire = b"".join(parts)
    fo = FR.frame_fragments(wire)[0]
    assert len(fo) - 1 == rec_frag[-1]
    out = {"wire": wire, "frag_start": fo[:-1].copy(), "frag_len": np.diff(fo.astype(np.int64)).astype(np.uint32),
           "rec_frag": np.array(rec_frag, np.uint64) if fragmented else None,
           "frag_pre": np.array(frag_pre, np.uint64) if fragmented else None,
           "rec_len": np.array(rec_len, np.uint32), "pay_pos": np.array(pay_pos, np.uint32),
           "pay_len": np.array(pay_len, np.uint32)}
    return out


def payload_extent(slot_off, pay_len, dst_cap):
    """The dst bytes place_copy may write: up to the last record's slice, or
    dst_cap (payload_plan.h payload_extent)."""
    n = len(pay_len)
    return min(int(slot_off[n - 1]) + int(pay_len[n - 1]), dst_cap)


def walk_positions(slot_off, n):
    """What place_copy walks: entry 0 at 0, entry r + 1 at slot_off[r], and the
    closing entry at 2^64 - 1."""
    return [0] + [int(x) for x in slot_off[:n]] + [U64]


KINDS = ("whole", "mid", "len1", "len15", "len16", "len17", "tail")


def choose_slices(heads, frag_len, names, seed=67):
    """Caller-chosen slices of the records of a heads model (rec_len,
    rec_frag, frag_pre): by turns the whole body, a slice that starts and ends
    inside a fragment, lengths 1, 15, 16 and 17, and a slice that ends on the
    record's last byte; the whole body of the two named long records; nothing
    of an empty record and of the records of the named run. -> (pay_pos,
    pay_len, kinds)."""
    rng = np.random.default_rng(seed)
    rec_len = heads["rec_len"]
    n = len(rec_len)
    pay_pos, pay_len, kinds = np.zeros(n, np.uint32), np.zeros(n, np.uint32), [""] * n
    for r in range(n):
        B = int(rec_len[r]) - 4
        if B <= 0 or names["run"] <= r < names["run"] + names["run_len"]:
            pay_pos[r] = int(rng.integers(0, 50))             # (ignored: no bytes)
            continue
        kind = "whole" if r in (names["ones"], names["long"]) else KINDS[r % len(KINDS)]
        want = {"len1": 1, "len15": 15, "len16": 16, "len17": 17}.get(kind)
        if kind == "mid":
            # inside fragments: not at a fragment's first byte, not behind its last
            lo, hi = int(heads["rec_frag"][r]), int(heads["rec_frag"][r + 1])
            inner = [j for j in range(lo, hi) if int(frag_len[j]) - 4 >= 3]
            if not inner:
                kind = "whole"
            else:
                ja, jb = inner[0], inner[-1]
                a = int(heads["frag_pre"][ja]) + 1
                b = int(heads["frag_pre"][jb]) + int(frag_len[jb]) - 4 - 1
                if ja == jb:
                    b = max(b, a + 1)
                x, ln = a, b - a
        if want is not None:
            ln = min(want, B)
            x = int(rng.integers(0, B - ln + 1))
        elif kind == "whole":
            x, ln = 0, B
        elif kind == "tail":
            ln = int(rng.integers(1, B + 1))
            x = B - ln
        pay_pos[r], pay_len[r], kinds[r] = 4 + x, ln, kind
    return pay_pos, pay_len, kinds


def pack_slots(pay_len, align):
    """onc_payload_slots' packing of given lengths: slot_off u64[n + 1]."""
    sizes = [round_up(x, align) for x in pay_len]
    return np.concatenate(([0], np.cumsum(sizes, dtype=np.uint64))).astype(np.uint64)


def odd_slots(pay_len, seed=71):
    """A caller's own list: non-decreasing, odd gaps before and between the
    slots, gaps after empty slices too. u64[n] and the capacity it needs."""
    rng = np.random.default_rng(seed)
    off, out = int(rng.integers(1, 40)), []
    for x in pay_len:
        out.append(off)
        off += int(x) + int(rng.choice((0, 0, 1, 3, 13, 16, 31, 100)))
    return np.array(out, np.uint64), off
