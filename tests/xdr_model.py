"""onc_xdr_unpack (include/onc_rpc.h) in plain Python: the contract's
pseudocode, record by record, with Python's unbounded integers (so nothing can
wrap here). tests/test_xdr_model.py pins it to tests/golden/xdr_args.json; the
host probe (tests/test_xdr_host.py) and the kernel (tests/test_gpu_xdr.py) are
compared with it.

A schema is a list of Field; descriptors are anything indexed by the names of
onc_msg's fields (dicts, or records of the numpy descriptor dtype)."""
from collections import namedtuple

U32, U64, BOOL, OPAQUE_FIXED, OPAQUE_VAR, ARRAY32, ARRAY64 = range(7)
SELECT, IF, NO_COLUMN = 0x100, 0x200, 0x400
EXACT = 0x1
OK, SKIPPED, BAD_EXTENT, SHORT, BAD_BOOL, TOO_LONG, TRAILING, HEAD_SHORT = range(8)
FIELDS_MAX = 64
RC_EINVAL = -1
MSG_CALL, MSG_REPLY, REPLY_ACCEPTED, ACCEPT_SUCCESS, ACCEPT_GARBAGE_ARGS = 0, 1, 0, 0, 4

Field = namedtuple("Field", "type_flags arg col_off cond_val reserved", defaults=(0, 0, 0, 0))


def pad4(x):
    return (x + 3) & ~3


def width(type_flags):
    return 4 if (type_flags & 0xFF) in (U32, BOOL, OPAQUE_FIXED) else 8


def layout(specs, n):
    """(type_flags, arg, cond_val) rows -> (fields with the columns of n records
    back to back, each 8-byte aligned; the bytes they take)."""
    fields, off = [], 0
    for tf, arg, cond in specs:
        if tf & NO_COLUMN:
            fields.append(Field(tf, arg, 0, cond))
        else:
            fields.append(Field(tf, arg, off, cond))
            off += (width(tf) * n + 7) & ~7
    return fields, off


def schema_check(fields, n, cols_cap):
    """onc_xdr_schema_check: 0, or the first bad field + 1."""
    if fields is None or len(fields) > FIELDS_MAX:
        return RC_EINVAL
    selected = False
    ranges = []
    for i, f in enumerate(fields):
        t = f.type_flags & 0xFF
        ok = t <= ARRAY64
        ok = ok and not (f.type_flags & ~(0xFF | SELECT | IF | NO_COLUMN)) and f.reserved == 0
        ok = ok and not ((f.type_flags & SELECT) and t not in (U32, BOOL))
        ok = ok and not ((f.type_flags & IF) and not selected)
        ok = ok and not (not (f.type_flags & IF) and f.cond_val != 0)
        ok = ok and not (t in (U32, U64, BOOL) and f.arg != 0)
        if ok and (f.type_flags & NO_COLUMN):
            ok = f.col_off == 0
        elif ok:
            w = width(f.type_flags) * n
            ok = f.col_off % (8 if t == U64 else 4) == 0 and f.col_off <= cols_cap and w <= cols_cap - f.col_off
            if ok and w:
                ok = all(not (f.col_off < b and a < f.col_off + w) for a, b in ranges)
                ranges.append((f.col_off, f.col_off + w))
        if not ok:
            return i + 1
        if f.type_flags & SELECT:
            selected = True
    return 0


def carries(status, m):
    if status != 0:
        return False
    if m["msg_type"] == MSG_CALL:
        return True
    return m["msg_type"] == MSG_REPLY and m["reply_stat"] == REPLY_ACCEPTED and m["stat"] == ACCEPT_SUCCESS


def be32(wire, at):
    return int.from_bytes(bytes(wire[at:at + 4]), "big")


def parse(read, fields, flags, L, base, o, hi, heads):
    """One record whose extent is good. read(p): the big-endian word at payload
    position p. -> (code, failing field, present, p, values): values[f] is the
    field's value, or (pos, len_or_count)."""
    p, sel, sel_ok, present = 0, 0, False, 0
    values = [0 if (f.type_flags & 0xFF) < OPAQUE_VAR else (0, 0) for f in fields]

    def need(k):
        if k > L - p:
            return SHORT
        if heads and k and o + p + k > hi:
            return HEAD_SHORT
        return OK

    for i, f in enumerate(fields):
        t = f.type_flags & 0xFF
        if (f.type_flags & IF) and not (sel_ok and sel == f.cond_val):
            if f.type_flags & SELECT:
                sel_ok = False
            continue
        v = 0
        if t in (U32, BOOL):
            if need(4):
                return need(4), i, present, 0, values
            v = read(p)
            if t == BOOL and v > 1:
                return BAD_BOOL, i, present, 0, values
            values[i] = v
            p += 4
        elif t == U64:
            if need(8):
                return need(8), i, present, 0, values
            values[i] = (read(p) << 32) | read(p + 4)
            p += 8
        elif t == OPAQUE_FIXED:
            if pad4(f.arg) > L - p:
                return SHORT, i, present, 0, values
            values[i] = base + p
            p += pad4(f.arg)
        else:
            if need(4):
                return need(4), i, present, 0, values
            c = read(p)
            if c > f.arg:
                return TOO_LONG, i, present, 0, values
            body = pad4(c) if t == OPAQUE_VAR else c * (4 if t == ARRAY32 else 8)
            if body > L - (p + 4):
                return SHORT, i, present, 0, values
            values[i] = (base + p + 4, c)
            p += 4 + body
        present |= 1 << i
        if f.type_flags & SELECT:
            sel, sel_ok = v, True
    if (flags & EXACT) and L - p != 0:
        return TRAILING, len(fields), present, 0, values
    return OK, 0, present, p, values


def unpack(wire, wire_len, msgs, status, fields, flags=0, rec_start=None, head_len=0, replies=None):
    """-> dict: xstat[n], present[n], rest_pos[n], rest_len[n], values[f][r],
    result[4], and garbage: the records whose reply gets GARBAGE_ARGS."""
    n = len(msgs)
    heads = rec_start is None and head_len != 0
    out = {"xstat": [], "present": [], "rest_pos": [], "rest_len": [], "garbage": [],
           "values": [[] for _ in fields], "result": [0, 0, 0, 0]}
    zero = [0 if (f.type_flags & 0xFF) < OPAQUE_VAR else (0, 0) for f in fields]
    for r in range(n):
        m = msgs[r]
        code, fail, present, base, p, L, values = SKIPPED, 0, 0, 0, 0, 0, zero
        if carries(int(status[r]), m):
            L, o = int(m["payload_len"]), int(m["payload_off"])
            if heads:
                lo = r * head_len
                hi = lo + head_len
                base = o - lo
                bad = o < lo or o > hi
            else:
                hi = wire_len
                bad = o > wire_len or L > wire_len - o
                base = o - int(rec_start[r]) if rec_start is not None else 0
                bad = bad or (rec_start is not None and o < int(rec_start[r]))
            bad = bad or base + L > 0xFFFFFFFF
            if bad:
                code, base, L = BAD_EXTENT, 0, 0
            else:
                code, fail, present, p, values = parse(lambda q: be32(wire, o + q), fields, flags, L, base, o, hi,
                                                       heads)
        good = code == OK
        if not good:                  # the failing field and every one after it write 0
            values = [v if (present >> i) & 1 else zero[i] for i, v in enumerate(values)]
        out["xstat"].append(code | (fail << 8))
        out["present"].append(present)
        out["rest_pos"].append(base + p if good else 0)
        out["rest_len"].append(L - p if good else 0)
        for i, v in enumerate(values):
            out["values"][i].append(v)
        out["result"][0 if good else (1 if SHORT <= code <= TRAILING else 2)] += 1
        if SHORT <= code <= TRAILING and m["msg_type"] == MSG_CALL:
            out["garbage"].append(r)
    return out


def cols_image(fields, n, cols_cap, values, fill=0xA5, extra=0):
    """The bytes of `cols` after the call: every element r < n of every column,
    and the fill everywhere else."""
    img = bytearray([fill]) * (cols_cap + extra)
    for f, vals in zip(fields, values):
        if f.type_flags & NO_COLUMN:
            continue
        t = f.type_flags & 0xFF
        for r, v in enumerate(vals):
            if t == U64:
                img[f.col_off + 8 * r:f.col_off + 8 * r + 8] = int(v).to_bytes(8, "little")
            elif t >= OPAQUE_VAR:
                img[f.col_off + 4 * r:f.col_off + 4 * r + 4] = int(v[0]).to_bytes(4, "little")
                at = f.col_off + 4 * n + 4 * r
                img[at:at + 4] = int(v[1]).to_bytes(4, "little")
            else:
                img[f.col_off + 4 * r:f.col_off + 4 * r + 4] = int(v).to_bytes(4, "little")
    return bytes(img)
