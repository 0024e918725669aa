"""tests/xdr_model.py (onc_xdr_unpack in plain Python) pinned to
tests/golden/xdr_args.json: argument blobs built with struct.pack and expected
columns written out by hand (tests/golden/make_xdr_args.py), independently of
the library. The host probe and the kernel are compared with the model."""
import json
import os

import xdr_model as M

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture():
    with open(os.path.join(HERE, "golden", "xdr_args.json")) as f:
        return json.load(f)


def place(records, header_len, gap=3):
    """The payloads in one wire, each behind header_len filler bytes, the
    records `gap` bytes apart -> (wire, descriptors, statuses, rec_start)."""
    wire, msgs, status, rec_start = bytearray(b"\xee" * gap), [], [], []
    for rec in records:
        pay = bytes.fromhex(rec["payload"])
        rec_start.append(len(wire))
        wire += b"\xee" * header_len
        msgs.append({"msg_type": rec["msg_type"], "reply_stat": rec.get("reply_stat", 0), "stat": rec.get("stat", 0),
                     "payload_off": len(wire), "payload_len": len(pay)})
        status.append(rec["status"])
        wire += pay + b"\xee" * gap
    return bytes(wire), msgs, status, rec_start


def _fields(schema, n):
    return M.layout([tuple(s) for s in schema], n)


def _norm(values):
    return [[tuple(v) if isinstance(v, (list, tuple)) else v for v in col] for col in values]


def _check(got, want, values):
    for k in ("xstat", "present", "rest_pos", "rest_len", "result", "garbage"):
        assert got[k] == want[k], k
    assert _norm(got["values"]) == _norm(values)


def test_write_args_rec_start_form():
    fx = _fixture()["write"]
    wire, msgs, status, rec_start = place(fx["records"], fx["header_len"])
    fields, cap = _fields(fx["schema"], len(msgs))
    assert M.schema_check(fields, len(msgs), cap) == 0
    plain = fx["expect"]["plain"]
    _check(M.unpack(wire, len(wire), msgs, status, fields, 0, rec_start=rec_start), plain, plain["values"])
    _check(M.unpack(wire, len(wire), msgs, status, fields, M.EXACT, rec_start=rec_start), fx["expect"]["exact"],
           plain["values"])


def test_setattr_args_payload_form():
    fx = _fixture()["setattr"]
    wire, msgs, status, _ = place(fx["records"], 0, gap=5)
    fields, cap = _fields(fx["schema"], len(msgs))
    assert M.schema_check(fields, len(msgs), cap) == 0
    for flags in (0, M.EXACT):                     # every record ends with its last field
        _check(M.unpack(wire, len(wire), msgs, status, fields, flags), fx["expect"], fx["expect"]["values"])


def test_heads_form_and_extents():
    fx = _fixture()["write"]
    a = bytes.fromhex(fx["records"][0]["payload"])
    fields, _ = _fields(fx["schema"], 4)
    # heads of 64 bytes: the payload starts 20 bytes into slot r; words past the slot are HEAD_SHORT
    head = 64
    wire = bytearray(4 * head)
    msgs, status = [], [0, 0, 0, 0]
    for r in range(4):
        wire[r * head + 20:(r + 1) * head] = a[:head - 20]
        msgs.append({"msg_type": 0, "reply_stat": 0, "stat": 0, "payload_off": r * head + 20, "payload_len": len(a)})
    msgs[1]["payload_off"] = head - 1              # before its slot
    msgs[2]["payload_off"] = 3 * head + 1          # past its slot's end
    msgs[3]["payload_off"] = 4 * head              # exactly at its slot's end: nothing of it is in the head
    got = M.unpack(bytes(wire), len(wire), msgs, status, fields, 0, head_len=head)
    # record 0: fh (4 + 32) and offset (8) fit the 44 payload bytes of the head; count ends at 48
    assert got["xstat"] == [M.HEAD_SHORT | 2 << 8, M.BAD_EXTENT, M.BAD_EXTENT, M.HEAD_SHORT | 0 << 8]
    assert got["present"] == [3, 0, 0, 0] and got["values"][0][0] == (24, 32) and got["values"][1][0] == 0x100000200
    assert got["garbage"] == [] and got["result"] == [0, 0, 4, 0]
    # the wire's end: an empty payload at wire_len is good, one byte further is not, nor a length one past the end
    w = a + b"\0" * 4
    n = len(a)
    ms = [{"msg_type": 0, "reply_stat": 0, "stat": 0, "payload_off": o, "payload_len": ln}
          for o, ln in ((n, 0), (n + 1, 0), (0, n + 1), ((1 << 64) - 1, 1), (0, n))]
    got = M.unpack(w, n, ms, [0] * 5, fields[:1], 0)
    assert got["xstat"] == [M.SHORT, M.BAD_EXTENT, M.BAD_EXTENT, M.BAD_EXTENT, M.OK]
    got = M.unpack(w, n, ms, [0] * 5, fields[:1], 0, rec_start=[n, 0, 0, 0, 1])
    assert got["xstat"] == [M.SHORT, M.BAD_EXTENT, M.BAD_EXTENT, M.BAD_EXTENT, M.BAD_EXTENT]


def test_schema_rules():
    F = M.Field
    ok = [F(M.OPAQUE_VAR, 64, 0), F(M.BOOL | M.SELECT, 0, 80), F(M.U64 | M.IF, 0, 120, 1), F(M.U32 | M.NO_COLUMN)]
    assert M.schema_check(ok, 10, 200) == 0 and M.schema_check([], 0, 0) == 0
    assert M.schema_check(ok, 10, 199) == 3                       # the last column ends at 200
    assert M.schema_check([F(7)], 1, 64) == 1
    assert M.schema_check(ok[:1] + [F(M.U64 | M.SELECT, 0, 80)], 10, 200) == 2
    assert M.schema_check([F(M.U32 | M.IF, 0, 0, 1)], 1, 64) == 1            # no selector before it
    assert M.schema_check([F(M.U32, 0, 0, 1)], 1, 64) == 1                   # cond_val without IF
    assert M.schema_check([F(M.U32, 5, 0)], 1, 64) == 1                      # arg on a type without one
    assert M.schema_check([F(M.U32 | M.NO_COLUMN, 0, 4)], 1, 64) == 1
    assert M.schema_check([F(M.U64, 0, 4)], 1, 64) == 1 and M.schema_check([F(M.U32, 0, 2)], 1, 64) == 1
    assert M.schema_check([F(M.U32, 0, 0), F(M.U32, 0, 36)], 10, 80) == 2    # [0, 40) and [36, 76)
    assert M.schema_check([F(M.U32, 0, 0), F(M.U32, 0, 40)], 10, 80) == 0
    assert M.schema_check([F(M.U32)] * 65, 0, 0) == M.RC_EINVAL
