"""Golden fixture for onc_xdr_unpack (Call arguments decoded into columns),
built here with struct.pack alone — no model, no library — so that
tests/xdr_model.py is pinned independently of both. Two NFSv3-shaped schemas
(RFC 1813) and a handful of argument blobs; the expected columns below were
written out by hand from the blobs' layout, not computed.

  WRITE3args   fh opaque<64>, offset hyper, count, stable (enum), data opaque<>
  SETATTR3args fh opaque<64>, sattr3 (four set_it optionals, two time_how
               three-way unions), sattrguard3 (an optional)

The WRITE records lie in a wire behind 44 filler bytes each (a Call's header
is not parsed by the call) and are addressed in the rec_start form, so their
positions count from the record's first byte; the SETATTR records are
addressed with neither rec_start nor heads: positions count from the payload.

Usage: python tests/golden/make_xdr_args.py  (writes xdr_args.json)
"""
import json
import os
import struct

U32, U64, BOOL, OPAQUE_FIXED, OPAQUE_VAR, ARRAY32, ARRAY64 = range(7)
SELECT, IF, NO_COLUMN = 0x100, 0x200, 0x400


def u32(*v):
    return b"".join(struct.pack(">I", x) for x in v)


def u64(v):
    return struct.pack(">Q", v)


def opaque(b):
    return u32(len(b)) + b + b"\0" * ((4 - len(b) % 4) % 4)


def write_args(fh, offset, count, stable, data):
    return opaque(fh) + u64(offset) + u32(count, stable) + opaque(data)


WRITE_SCHEMA = [[OPAQUE_VAR, 64, 0], [U64, 0, 0], [U32, 0, 0], [U32, 0, 0], [OPAQUE_VAR, 0xFFFFFFFF, 0]]

SETATTR_SCHEMA = [
    [OPAQUE_VAR, 64, 0],                                       # 0 object
    [BOOL | SELECT, 0, 0], [U32 | IF, 0, 1],                   # 1, 2 mode
    [BOOL | SELECT, 0, 0], [U32 | IF, 0, 1],                   # 3, 4 uid
    [BOOL | SELECT, 0, 0], [U32 | IF, 0, 1],                   # 5, 6 gid
    [BOOL | SELECT, 0, 0], [U64 | IF, 0, 1],                   # 7, 8 size
    [U32 | SELECT, 0, 0], [U32 | IF, 0, 2], [U32 | IF, 0, 2],  # 9, 10, 11 atime: SET_TO_CLIENT_TIME = 2
    [U32 | SELECT, 0, 0], [U32 | IF, 0, 2], [U32 | IF, 0, 2],  # 12, 13, 14 mtime
    [BOOL | SELECT, 0, 0], [U32 | IF, 0, 1], [U32 | IF, 0, 1],  # 15, 16, 17 guard: check, obj_ctime
]


def main():
    hdr = 44
    a = write_args(b"\x01" * 32, 0x0000000100000200, 10, 2, b"\xd0" * 10)          # 68 bytes
    b = write_args(b"\x02" * 7, 5, 3, 0, b"\xd1" * 3) + b"\xee" * 4               # 36 bytes + 4 that nobody parses
    c = a[:50]                                                                     # cut inside `stable`
    d = opaque(b"\x03" * 65) + a[36:]                                              # a 65-byte handle
    assert (len(a), len(b), len(d)) == (68, 40, 104)
    write_recs = [
        {"msg_type": 0, "status": 0, "payload": a.hex()},
        {"msg_type": 0, "status": 0, "payload": b.hex()},
        {"msg_type": 0, "status": 0, "payload": c.hex()},
        {"msg_type": 0, "status": 0, "payload": d.hex()},
        {"msg_type": 1, "reply_stat": 1, "status": 0, "payload": a.hex()},        # a denied reply: no payload
        {"msg_type": 0, "status": 13, "payload": a.hex()},                        # a record that failed to decode
        {"msg_type": 1, "reply_stat": 0, "stat": 0, "status": 0, "payload": b.hex()},   # a Success reply
    ]
    write_expect = {
        # positions count from the record: 44 bytes of header before the payload
        "plain": {
            "xstat": [0, 0, 3 | 3 << 8, 5 | 0 << 8, 1, 1, 0],
            "present": [31, 31, 7, 0, 0, 0, 31],
            "rest_pos": [112, 80, 0, 0, 0, 0, 80],
            "rest_len": [0, 4, 0, 0, 0, 0, 4],
            "values": [
                [[48, 32], [48, 7], [48, 32], [0, 0], [0, 0], [0, 0], [48, 7]],                # fh
                [0x100000200, 5, 0x100000200, 0, 0, 0, 5],                                      # offset
                [10, 3, 10, 0, 0, 0, 3],                                                        # count
                [2, 0, 0, 0, 0, 0, 0],                                                          # stable
                [[100, 10], [76, 3], [0, 0], [0, 0], [0, 0], [0, 0], [76, 3]],                 # data
            ],
            "result": [3, 2, 2, 0],
            "garbage": [2, 3],
        },
        # ONC_XDR_EXACT: the four bytes behind b's data are an error at field 5; the columns stay
        "exact": {
            "xstat": [0, 6 | 5 << 8, 3 | 3 << 8, 5, 1, 1, 6 | 5 << 8],
            "present": [31, 31, 7, 0, 0, 0, 31],
            "rest_pos": [112, 0, 0, 0, 0, 0, 0],
            "rest_len": [0, 0, 0, 0, 0, 0, 0],
            "values": None,                                                                     # as "plain"
            "result": [1, 4, 2, 0],
            "garbage": [1, 2, 3],                                                               # (6 is a reply)
        },
    }
    s1 = (opaque(b"\x11" * 8) + u32(1, 0o644) + u32(0) + u32(1, 100) + u32(1) + u64((1 << 33) + 5) +
          u32(2, 1000, 7) + u32(1) + u32(0))
    s2 = (opaque(b"\x12" * 5) + u32(0) + u32(1, 0) + u32(0) + u32(0) + u32(0) + u32(2, 0xFFFFFFFF, 999999999) +
          u32(1, 5, 6))
    s3 = opaque(b"\x13" * 4) + u32(2)                              # set_it = 2: not a bool
    s4 = opaque(b"") + u32(0, 0, 0, 0) + u32(3) + u32(0) + u32(0)  # time_how = 3: no arm matches, nothing follows it
    assert (len(s1), len(s2), len(s3), len(s4)) == (64, 60, 12, 32)
    setattr_recs = [{"msg_type": 0, "status": 0, "payload": s.hex()} for s in (s1, s2, s3, s4)]
    z = 0
    setattr_expect = {
        "xstat": [0, 0, 4 | 1 << 8, 0],
        "present": [40943, 258747, 1, 37547],
        "rest_pos": [64, 60, 0, 32],
        "rest_len": [0, 0, 0, 0],
        "values": [
            [[4, 8], [4, 5], [4, 4], [4, 0]],
            [1, 0, z, 0], [420, 0, z, 0],
            [0, 1, z, 0], [0, 0, z, 0],
            [1, 0, z, 0], [100, 0, z, 0],
            [1, 0, z, 0], [(1 << 33) + 5, 0, z, 0],
            [2, 0, z, 3], [1000, 0, z, 0], [7, 0, z, 0],
            [1, 2, z, 0], [0, 0xFFFFFFFF, z, 0], [0, 999999999, z, 0],
            [0, 1, z, 0], [0, 5, z, 0], [0, 6, z, 0],
        ],
        "result": [3, 1, 0, 0],
        "garbage": [2],
    }
    fx = {
        "source": "tests/golden/make_xdr_args.py (struct.pack; no model, no library): include/onc_rpc.h "
                  "onc_xdr_unpack; RFC 4506 (XDR), RFC 1813 WRITE3args / SETATTR3args; reference opaque.rs:76-95",
        "write": {"schema": WRITE_SCHEMA, "header_len": hdr, "records": write_recs, "expect": write_expect},
        "setattr": {"schema": SETATTR_SCHEMA, "records": setattr_recs, "expect": setattr_expect},
    }
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "xdr_args.json")
    with open(path, "w") as f:
        json.dump(fx, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
