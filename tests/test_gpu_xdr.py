"""onc_xdr_unpack on the device against tests/xdr_model.py: every output —
the columns' bytes, xstat, present, rest_pos, rest_len, the replies, result —
compared whole and bit-exactly, the outputs pre-filled with a sentinel and
guard words behind them, the optional outputs given and not given."""
import struct

import numpy as np
import pytest

import onc_rpc_amd.layout as L
import xdr_model as M

pytestmark = pytest.mark.gpu
T = 0xFFFFFFFF
HDR = 44            # mark, xid, msg_type, rpcvers, program, version, procedure, two AUTH_NONE auths


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codec(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = R.Codec(0)
    yield c
    c.close()


def u32(*v):
    return b"".join(struct.pack(">I", x) for x in v)


def opaque(b):
    return u32(len(b)) + b + b"\0" * ((4 - len(b) % 4) % 4)


def call_header(xid, body_len):
    return u32((HDR - 4 + body_len) | 0x80000000, xid, 0, 2, 100003, 3, 7, 0, 0, 0, 0)


SPECS = {
    "none": [],
    "u32": [(M.U32, 0, 0)],
    "u64": [(M.U64, 0, 0)],
    "bool": [(M.BOOL, 0, 0)],
    "fixed": [(M.OPAQUE_FIXED, 6, 0)],
    "var": [(M.OPAQUE_VAR, 40, 0)],
    "array32": [(M.ARRAY32, 5, 0)],
    "array64": [(M.ARRAY64, 3, 0)],
    "all": [(M.U32, 0, 0), (M.U64, 0, 0), (M.BOOL | M.SELECT, 0, 0), (M.U32 | M.IF, 0, 1), (M.OPAQUE_FIXED, 6, 0),
            (M.OPAQUE_VAR, 40, 0), (M.ARRAY32, 4, 0), (M.ARRAY64, 4, 0), (M.U32, 0, 0)],
    "sixty_four": [(M.U32 | M.SELECT, 0, 0)] + [((M.U32, M.U64, M.BOOL)[i % 3] | (M.IF if i % 5 == 0 else 0), 0,
                                                 i % 3 if i % 5 == 0 else 0) for i in range(63)],
    "no_column": [(t | M.NO_COLUMN, a, 0) for t, a in ((M.U32, 0), (M.U64, 0), (M.BOOL, 0), (M.OPAQUE_FIXED, 5),
                                                         (M.OPAQUE_VAR, 9), (M.ARRAY32, 2), (M.ARRAY64, 2))] +
                 [(M.U32, 0, 0)],
    # present and absent arms, a SELECT field that is itself absent, two arms of one selector
    "select": [(M.BOOL | M.SELECT, 0, 0), (M.U64 | M.IF, 0, 1), (M.U32 | M.SELECT | M.IF, 0, 1), (M.U32 | M.IF, 0, 7),
               (M.U32 | M.SELECT, 0, 0), (M.OPAQUE_VAR | M.IF, 12, 1), (M.U64 | M.IF, 0, 2), (M.U32 | M.IF, 0, 2),
               (M.U32, 0, 0)],
}


def gen_payload(fields, rng, hostile=0.0):
    """A payload that parses against the schema (selectors drawn from the arms'
    values), or with probability `hostile` per field one that goes wrong there."""
    out, sel, sel_ok = b"", 0, False
    conds = sorted({f.cond_val for f in fields if f.type_flags & M.IF} | {0, 1})
    for f in fields:
        t = f.type_flags & 0xFF
        if (f.type_flags & M.IF) and not (sel_ok and sel == f.cond_val):
            if f.type_flags & M.SELECT:
                sel_ok = False
            continue
        bad = rng.random() < hostile
        v = 0
        if t == M.U32:
            v = int(rng.choice(conds)) if f.type_flags & M.SELECT else int(rng.integers(0, 1 << 32))
            if bad and f.type_flags & M.SELECT:
                v = int(rng.choice([2, T, 0x80000000]))
            out += u32(v)
        elif t == M.BOOL:
            v = int(rng.choice([2, T, 0x100])) if bad else int(rng.integers(0, 2))
            out += u32(v)
        elif t == M.U64:
            out += struct.pack(">Q", int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)))
        elif t == M.OPAQUE_FIXED:
            out += bytes(rng.integers(1, 255, M.pad4(f.arg), dtype=np.uint8))
        else:
            unit = {M.OPAQUE_VAR: 1, M.ARRAY32: 4, M.ARRAY64: 8}[t]
            c = int(rng.integers(0, min(f.arg, 40) + 1))
            body = bytes(rng.integers(1, 255, M.pad4(c * unit), dtype=np.uint8))
            if bad:
                c = int(rng.choice([f.arg + 1, T - 2, T - 1, T, 0x40000000, 0x20000000, c + 5]))
            out += u32(c) + body
        if f.type_flags & M.SELECT:
            sel, sel_ok = v, True
    if rng.random() < hostile:
        out = out[:int(rng.integers(0, len(out) + 1))]
    elif rng.random() < 0.2:
        out += b"\x77" * int(rng.choice([1, 4, 8]))
    return out


class Batch:
    """Payloads laid into one wire behind a header each, at every alignment."""

    def __init__(self, payloads, rng=None, kinds=None, header=HDR):
        wire = bytearray()
        n = len(payloads)
        self.msgs = np.zeros(n, L.MSG_DTYPE)
        self.status = np.zeros(n, np.int32)
        self.rec_start = np.zeros(n, np.uint64)
        for r, pay in enumerate(payloads):
            wire += b"\xee" * (int(rng.integers(0, 17)) if rng is not None else (r * 5) % 16)
            self.rec_start[r] = len(wire)
            wire += call_header(r + 1, len(pay))[:header]
            m = self.msgs[r]
            m["xid"], m["payload_off"], m["payload_len"] = r + 1, len(wire), len(pay)
            kind = kinds[r] if kinds is not None else "call"
            if kind == "reply":
                m["msg_type"] = 1
            elif kind == "denied":
                m["msg_type"], m["reply_stat"] = 1, 1
            elif kind == "not_success":
                m["msg_type"], m["stat"] = 1, 1 + r % 5
            elif kind == "failed":
                self.status[r] = 1 + r % 13
                self.msgs[r:r + 1].view(np.uint8)[:] = rng.integers(0, 256, 64, dtype=np.uint8)
            wire += pay
        self.wire = np.frombuffer(bytes(wire), np.uint8)


def skeletons(msgs):
    """What onc_route_calls leaves for served Calls, in the records' order."""
    rep = np.zeros(len(msgs), L.MSG_DTYPE)
    rep["xid"], rep["msg_type"] = msgs["xid"], 1
    return rep


def check(R, codec, wire, msgs, status, fields, cap, flags=0, rec_start=None, head_len=0, wire_len=None, tag="",
          options=((True, True, True), (False, False, False), (True, False, False), (False, True, True))):
    """One call per combination of (present, rest, replies) against the model."""
    n = len(msgs)
    wl = len(wire) if wire_len is None else wire_len
    host = wire if isinstance(wire, np.ndarray) else None
    want = M.unpack(host if host is not None else wire.host_bytes, wl, msgs, status, fields, flags, rec_start, head_len)
    extra = 4
    image = M.cols_image(fields, n, cap, want["values"], 0xA5, 8 * extra)
    frows = np.array([tuple(f) for f in fields], L.XDR_FIELD_DTYPE) if fields else np.zeros(0, L.XDR_FIELD_DTYPE)
    skel = skeletons(msgs)
    for present, rest, replies in options:
        got = R.xdr_unpack_host(codec, wire if host is not None else wire.dev, msgs, status, frows, cap, flags=flags,
                                rec_start=rec_start, head_len=head_len, present=present, rest=rest,
                                replies=skel if replies else None, wire_len=wl, extra=extra)
        raw = got["raw"]
        where = (tag, n, flags, present, rest, replies)
        assert raw["cols"].tobytes() == image, where
        assert raw["xstat"].tolist() == want["xstat"] + [T] * extra, where
        assert raw["result"].tolist() == want["result"] + [(1 << 64) - 1] * extra, where
        if present:
            assert raw["present"].tolist() == want["present"] + [(1 << 64) - 1] * extra, where
        if rest:
            assert raw["rest_pos"].tolist() == want["rest_pos"] + [T] * extra, where
            assert raw["rest_len"].tolist() == want["rest_len"] + [T] * extra, where
        if replies:
            patched = skel.copy()
            patched["stat"][want["garbage"]] = M.ACCEPT_GARBAGE_ARGS
            assert raw["replies"][:n * 64].tobytes() == patched.tobytes(), where       # exactly the stat byte changes
            assert (raw["replies"][n * 64:] == 0xA5).all(), where
    return want


def codes(want):
    return {x & 0xFF for x in want["xstat"]}


def test_sizes_around_the_tile_and_every_schema(R, codec):
    rng = np.random.default_rng(11)
    kinds_all = ["call"] * 12 + ["reply", "reply", "denied", "not_success", "failed", "failed"]
    seen = set()
    for n in (0, 1, 63, 64, 65, R.XDR_TILE - 1, R.XDR_TILE, R.XDR_TILE + 1):
        for name, specs in SPECS.items():
            fields, cap = M.layout(specs, n)
            assert M.schema_check(fields, n, cap) == 0, name
            pays = [gen_payload(fields, rng, hostile=0.04) for _ in range(n)]
            kinds = [kinds_all[int(k)] for k in rng.integers(0, len(kinds_all), n)]
            b = Batch(pays, rng, kinds)
            form = int(rng.integers(0, 2))
            opts = ((True, True, True), (False, False, False)) if n not in (65, R.XDR_TILE + 1) else \
                ((True, False, False), (False, True, True))
            want = check(R, codec, b.wire, b.msgs, b.status, fields, cap, flags=int(rng.integers(0, 2)),
                         rec_start=b.rec_start if form else None, tag=name, options=opts)
            seen |= codes(want)
    assert {M.OK, M.SKIPPED, M.SHORT, M.BAD_BOOL, M.TOO_LONG, M.TRAILING} <= seen


def test_truncation_sweep_at_every_alignment(R, codec):
    specs = SPECS["all"]
    blob = (u32(0xDEADBEEF) + struct.pack(">Q", 0x0102030405060708) + u32(1, 0x11223344) + b"\xf1" * 6 + b"\0\0" +
            opaque(b"\xa7" * 25) + u32(3, 5, 6, 7) + u32(2) + struct.pack(">QQ", 1 << 63, 9) + u32(0xCAFEF00D))
    assert len(blob) == 100
    pays, pad = [], []
    for cut in range(len(blob) + 1):
        for mis in range(16):
            pays.append(blob[:cut])
            pad.append(mis)
    n = len(pays)
    fields, cap = M.layout(specs, n)
    # every cut at every payload_off mod 16: the header length makes up the difference
    wire = bytearray()
    msgs, rec_start = np.zeros(n, L.MSG_DTYPE), np.zeros(n, np.uint64)
    for r, (pay, mis) in enumerate(zip(pays, pad)):
        wire += b"\xee" * ((-len(wire)) % 16)
        rec_start[r] = len(wire)
        wire += b"\xee" * (32 + mis)
        msgs[r]["xid"], msgs[r]["payload_off"], msgs[r]["payload_len"] = r, len(wire), len(pay)
        assert len(wire) % 16 == mis
        wire += pay
    w = np.frombuffer(bytes(wire), np.uint8)
    st = np.zeros(n, np.int32)
    for flags in (0, M.EXACT):
        want = check(R, codec, w, msgs, st, fields, cap, flags=flags, rec_start=rec_start, tag="sweep",
                     options=((True, True, True),))
        assert want["result"] == [16, n - 16, 0, 0] and codes(want) == {M.OK, M.SHORT}
    assert 1600 <= n <= 2100


def test_hostile_lengths_counts_bools_and_selectors(R, codec):
    pays, specs = [], [(M.BOOL | M.SELECT, 0, 0), (M.U32 | M.IF, 0, 1), (M.U32 | M.SELECT, 0, 0),
                       (M.OPAQUE_VAR | M.IF, 16, 2), (M.ARRAY32 | M.IF, T, 3), (M.ARRAY64 | M.IF, T, 4),
                       (M.OPAQUE_VAR | M.IF, T, 5), (M.U32, 0, 0)]
    tail = b"\x33" * 24
    for b in (0, 1, 2, T):
        head = u32(b) + (u32(7) if b == 1 else b"")
        for s in (0, 1, 2, 3, 4, 5, T):
            pays.append(head + u32(s) + u32(9))
        for ln in (0, 15, 16, 17, T - 2, T - 1, T):
            pays.append(head + u32(2, ln) + tail)
        for sel, vals in ((3, (0, 5, 6, 7, 0x40000000, 0x40000001, 0x80000000, T)),
                          (4, (0, 2, 3, 4, 0x20000000, 0x20000001, 0x80000000, T)), (5, (20, 21, T - 2, T - 1, T))):
            for c in vals:
                pays.append(head + u32(sel, c) + tail)
    fields, cap = M.layout(specs, len(pays))
    b = Batch(pays)
    for flags in (0, M.EXACT):
        want = check(R, codec, b.wire, b.msgs, b.status, fields, cap, flags=flags, rec_start=b.rec_start, tag="hostile",
                     options=((True, True, True), (False, False, False)))
        assert {M.OK, M.SHORT, M.BAD_BOOL, M.TOO_LONG} <= codes(want)
    assert M.TRAILING in codes(want)


def test_records_that_carry_no_payload(R, codec):
    rng = np.random.default_rng(5)
    fields, cap = M.layout(SPECS["all"], 200)
    kinds = [("call", "failed", "denied", "not_success", "reply")[int(k)] for k in rng.integers(0, 5, 200)]
    b = Batch([gen_payload(fields, rng) for _ in range(200)], rng, kinds)
    want = check(R, codec, b.wire, b.msgs, b.status, fields, cap, rec_start=b.rec_start, tag="skipped")
    assert want["result"][2] == sum(k in ("failed", "denied", "not_success") for k in kinds) > 20
    assert want["garbage"] == []
    # nothing but failed records: descriptors of random bytes are never looked at
    b = Batch([b""] * 70, rng, ["failed"] * 70)
    check(R, codec, b.wire, b.msgs, b.status, fields[:3], cap, tag="all failed")


def test_extents_are_checked_before_any_read(R, codec):
    rng = np.random.default_rng(9)
    fields, cap = M.layout(SPECS["var"] + SPECS["u32"], 12)
    good = opaque(b"\x42" * 9) + u32(77)
    b = Batch([good] * 12, rng)
    wl = len(b.wire)
    m = b.msgs
    m[1]["payload_off"], m[1]["payload_len"] = wl, 0                    # the empty slice at the end: good, then SHORT
    m[2]["payload_off"], m[2]["payload_len"] = wl + 1, 0
    m[3]["payload_len"] = wl - int(m[3]["payload_off"]) + 1             # one past the end
    m[4]["payload_off"] = (1 << 64) - 1
    m[5]["payload_off"], m[5]["payload_len"] = (1 << 64) - 1, 0
    m[6]["payload_off"] = int(b.rec_start[6]) - 1                       # before its record (rec_start form only)
    m[7]["payload_len"] = T
    m[8]["payload_off"], m[8]["payload_len"] = wl - 4, 4                # the last word of the wire
    for rs in (b.rec_start, None):
        want = check(R, codec, b.wire, m, b.status, fields, cap, rec_start=rs, tag="extents")
        bad = [r for r, x in enumerate(want["xstat"]) if x & 0xFF == M.BAD_EXTENT]
        assert bad == ([2, 3, 4, 5, 6, 7] if rs is not None else [2, 3, 4, 5, 7])
        assert want["xstat"][1] == M.SHORT
    # a wire_len below the true size cuts the readable window
    cut = int(m[9]["payload_off"]) + 6
    want = check(R, codec, b.wire, m, b.status, fields, cap, wire_len=cut, tag="short wire",
                 options=((True, True, True),))
    assert want["xstat"][9] == M.BAD_EXTENT and want["xstat"][0] == M.OK


def _write_batch(rng, n):
    specs = [(M.OPAQUE_VAR, 64, 0), (M.U64, 0, 0), (M.U32, 0, 0), (M.U32, 0, 0), (M.OPAQUE_VAR, T, 0)]
    datas = [bytes(rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8)) for _ in range(n)]
    pays = [opaque(bytes(rng.integers(0, 256, int(rng.integers(0, 65)), dtype=np.uint8))) +
            struct.pack(">Q", int(rng.integers(0, 1 << 62))) + u32(len(d), int(rng.integers(0, 3))) + opaque(d)
            for d in datas]
    return specs, datas, pays


def test_rec_start_form_feeds_place_payloads(R, codec):
    rng = np.random.default_rng(21)
    n = 150
    specs, datas, pays = _write_batch(rng, n)
    pays[7] = pays[7][:20]                                               # one that does not parse: no slice
    fields, cap = M.layout(specs, n)
    b = Batch(pays, rng)
    rec_len = np.array([HDR + len(p) for p in pays], np.uint32)
    dec = R.decode_host_extents(codec, b.wire, b.rec_start, rec_len, L.DECODE_SLICE)
    msgs, status = dec[0], dec[2]
    assert (status == 0).all() and np.array_equal(msgs["payload_off"], b.msgs["payload_off"])
    want = check(R, codec, b.wire, msgs, status, fields, cap, flags=M.EXACT, rec_start=b.rec_start, tag="write",
                 options=((True, True, True),))
    frows = np.array([tuple(f) for f in fields], L.XDR_FIELD_DTYPE)
    got = R.xdr_unpack_host(codec, b.wire, msgs, status, frows, cap, flags=M.EXACT, rec_start=b.rec_start)
    col = got["cols"][fields[4].col_off:fields[4].col_off + 8 * n].view(np.uint32)
    pay_pos, pay_len = col[:n].copy(), col[n:].copy()
    assert [int(x) for x in pay_len] == [len(d) if r != 7 else 0 for r, d in enumerate(datas)]
    slot = np.concatenate([[0], np.cumsum((pay_len.astype(np.uint64) + 63) // 64 * 64)]).astype(np.uint64)
    placed = R.place_payloads_host(codec, b.wire.tobytes(), b.rec_start, rec_len, None, None, rec_len, pay_pos, pay_len,
                                   slot[:n], int(slot[n]), guard=64)
    for r, d in enumerate(datas):
        if r != 7:
            assert placed[64 + int(slot[r]):64 + int(slot[r]) + len(d)].tobytes() == d, r
    assert want["xstat"][7] & 0xFF == M.SHORT


@pytest.mark.parametrize("head_len", [64, 160])
def test_heads_form_after_defragment_heads(R, codec, head_len):
    rng = np.random.default_rng(head_len)
    n = 90
    specs, datas, pays = _write_batch(rng, n)
    specs, pays = specs + [(M.U32, 0, 0)], [p + u32(r) for r, p in enumerate(pays)]   # a word behind the data: whether
    fields, cap = M.layout(specs, n)                                                   # it lies in the head varies
    wire, start, length = bytearray(), [], []
    for r, p in enumerate(pays):
        wire += b"\xee" * int(rng.integers(0, 9))
        start.append(len(wire))
        wire += call_header(r + 1, len(p)) + p
        length.append(HDR + len(p))
    heads = R.defragment_host_heads(codec, bytes(wire), start, length, head_len)
    assert int(heads["result"][0]) == n and (heads["status"] == 0).all()
    dec = R.decode_host_heads(codec, heads["heads"].tobytes(), head_len, heads["rec_len"], L.DECODE_SLICE)
    msgs, status = dec[0], dec[2]
    assert (status == 0).all()
    want = check(R, codec, heads["heads"], msgs, status, fields, cap, head_len=head_len, tag="heads",
                 options=((True, True, True), (False, False, False)))
    assert codes(want) == ({M.HEAD_SHORT} if head_len == 64 else {M.OK, M.HEAD_SHORT})
    assert want["garbage"] == [] and want["result"][1] == 0
    for r in range(n):                                                    # positions count from the head slot
        if want["xstat"][r] == M.OK:
            assert want["values"][4][r] == (HDR + len(pays[r]) - 4 - M.pad4(len(datas[r])), len(datas[r]))
            assert want["values"][5][r] == r
    # a payload_off outside its slot
    msgs = msgs.copy()
    msgs[3]["payload_off"] = 3 * head_len - 1
    msgs[4]["payload_off"] = 5 * head_len + 1
    msgs[5]["payload_off"] = 6 * head_len
    want = check(R, codec, heads["heads"], msgs, status, fields, cap, head_len=head_len, tag="heads extents",
                 options=((True, True, True),))
    assert [want["xstat"][r] & 0xFF for r in (3, 4, 5)] == [M.BAD_EXTENT, M.BAD_EXTENT, M.HEAD_SHORT]


class Mapped:
    """A wire in mapped host memory."""

    def __init__(self, R, codec, data):
        self.m = R.HostMapped.from_array(codec, np.frombuffer(data, np.uint8))
        self.dev = self.m
        self.host_bytes = data


def test_wire_in_mapped_host_memory(R, codec):
    rng = np.random.default_rng(31)
    fields, cap = M.layout(SPECS["all"], 300)
    b = Batch([gen_payload(fields, rng, hostile=0.03) for _ in range(300)], rng)
    w = Mapped(R, codec, b.wire.tobytes())
    try:
        want = check(R, codec, w, b.msgs, b.status, fields, cap, rec_start=b.rec_start, wire_len=len(b.wire),
                     tag="mapped", options=((True, True, True),))
        assert M.OK in codes(want)
    finally:
        w.m.close()


G31, G32 = 1 << 31, 1 << 32
FAR = G32 + G31 + 5


class Far:
    """A wire based FAR bytes into a slab that is allocated and never filled."""

    def __init__(self, slab, data):
        import torch
        self.dev = slab.data_ptr() + FAR
        slab[FAR:FAR + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
        self.host_bytes = data


def test_wire_beyond_4_gib(R, codec):
    import torch
    size = FAR + (1 << 20)
    free = torch.cuda.mem_get_info()[0]
    if free < size + (1 << 30):
        pytest.skip(f"needs {size + (1 << 30)} bytes of free device memory, {free} are free")
    slab = torch.empty(size, dtype=torch.uint8, device="cuda")
    try:
        rng = np.random.default_rng(41)
        fields, cap = M.layout(SPECS["all"], 300)
        b = Batch([gen_payload(fields, rng, hostile=0.03) for _ in range(300)], rng)
        # the wire based far into the slab ...
        w = Far(slab, b.wire.tobytes())
        want = check(R, codec, w, b.msgs, b.status, fields, cap, rec_start=b.rec_start, wire_len=len(b.wire), tag="far base",
                     options=((True, True, True),))
        assert M.OK in codes(want)
        # ... and the slab as the wire, the offsets beyond 2^32 + 2^31
        msgs = b.msgs.copy()
        msgs["payload_off"] += np.uint64(FAR)
        got = R.xdr_unpack_host(codec, slab, msgs, b.status, np.array([tuple(f) for f in fields], L.XDR_FIELD_DTYPE), cap,
                                rec_start=b.rec_start + np.uint64(FAR), wire_len=size)
        assert got["xstat"].tolist() == want["xstat"] and got["rest_pos"].tolist() == want["rest_pos"]
        assert got["cols"].tobytes() == M.cols_image(fields, 300, cap, want["values"])
    finally:
        del slab
        torch.cuda.empty_cache()


def test_cpp_mirror(tmp_path):
    """XdrSchema / unpack_args / UnpackedArgs of include/onc_rpc.hpp
    (tests/cpp_xdr/test_xdr.cpp) over a stream written here; its summary is
    compared with the model's."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "tests", "cpp_xdr", "test_xdr")
    assert os.path.exists(exe), "build() compiles tests/cpp_xdr"
    rng = np.random.default_rng(77)
    write_specs = [(M.OPAQUE_VAR, 64, 0), (M.U64, 0, 0), (M.U32, 0, 0), (M.U32, 0, 0), (M.OPAQUE_VAR, T, 0)]
    other_specs = [(M.OPAQUE_VAR | M.NO_COLUMN, 64, 0), (M.BOOL | M.SELECT, 0, 0), (M.U64 | M.IF, 0, 1),
                   (M.U32 | M.SELECT, 0, 0), (M.U32 | M.IF, 0, 2), (M.U32 | M.IF, 0, 2)]
    _, _, wpays = _write_batch(rng, 40)
    wire, recs = bytearray(), []                        # (procedure, payload), in stream order
    for r in range(90):
        proc = int(rng.choice([7, 7, 2, 5]))
        if proc == 7:
            pay = wpays[r % 40]
            if r % 6 == 0:
                pay = pay[:int(rng.integers(0, len(pay)))]
            elif r % 11 == 0:
                pay += b"\0" * 4                        # ONC_XDR_EXACT: trailing bytes
        else:
            fields, _ = M.layout(other_specs, 1)
            pay = gen_payload(fields, rng, hostile=0.1)
        recs.append((proc, pay))
        wire += u32((HDR - 4 + len(pay)) | 0x80000000, 1000 + r, 0, 2, 100003, 3, proc, 0, 0, 0, 0) + pay
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(bytes(wire))
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS test_xdr" in r.stdout, r.stdout + r.stderr
    out = outp.read_bytes()
    at = 0
    for proc, specs, flags, row in ((7, write_specs, M.EXACT, "<IIQIIII"), (2, other_specs, 0, "<IQIII")):
        idx = [i for i, (p, _) in enumerate(recs) if p == proc]
        n = len(idx)
        fields, _ = M.layout(specs, n)
        pays = [recs[i][1] for i in idx]
        b = Batch(pays)
        want = M.unpack(b.wire, len(b.wire), b.msgs, b.status, fields, flags)      # positions from the payload
        assert struct.unpack_from("<Q", out, at)[0] == n
        at += 8
        for k in range(n):
            common = struct.unpack_from("<IIQIII", out, at)
            at += struct.calcsize("<IIQIII")
            stat = M.ACCEPT_GARBAGE_ARGS if k in want["garbage"] else 0
            assert common == (idx[k], want["xstat"][k], want["present"][k], want["rest_pos"][k], want["rest_len"][k],
                              stat), (proc, k)
            cols = struct.unpack_from(row, out, at)
            at += struct.calcsize(row)
            v = [want["values"][f][k] for f in range(len(fields))]
            if proc == 7:
                assert cols == (v[0][0], v[0][1], v[1], v[2], v[3], v[4][0], v[4][1]), (proc, k)
            else:
                assert cols == (v[1], v[2], v[3], v[4], v[5]), (proc, k)
        assert want["garbage"], "some arguments do not parse"
    assert at == len(out)


def test_graph_capture_and_replay(R):
    """The call is kernel launches only: captured once, replayed on two inputs;
    without the reserve it would grow its scratch inside the capture and is
    refused with nothing launched."""
    import torch
    rng = np.random.default_rng(3)
    n = 2 * R.XDR_TILE + 77
    fields, cap = M.layout(SPECS["all"], n)
    frows = np.array([tuple(f) for f in fields], L.XDR_FIELD_DTYPE)
    batches = [Batch([gen_payload(fields, rng, hostile=0.05) for _ in range(n)], rng) for _ in range(2)]
    wl = max(len(b.wire) for b in batches)
    d_wire = torch.zeros(wl + 16, dtype=torch.uint8, device="cuda")
    d_msgs = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_rs = torch.zeros(n, dtype=torch.int64, device="cuda")
    cols = torch.full((cap + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    xstat = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    present = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    rest_pos = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    rest_len = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    outs = (xstat, present, rest_pos, rest_len, res)
    s = torch.cuda.Stream()

    def work(codec):
        codec.xdr_unpack(d_wire, wl, d_msgs, d_st, n, frows, cols, xstat, res, rec_start=d_rs, present=present,
                         rest_pos=rest_pos, rest_len=rest_len, cols_cap=cap)

    fresh = R.Codec(0, stream=s.cuda_stream)
    codec = R.Codec(0, stream=s.cuda_stream)
    try:
        err = None
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            try:
                work(fresh)
            except R.CodecError as e:
                err = str(e)
        assert err is not None and "rc=-5" in err, err
        torch.cuda.synchronize()
        assert all((t == -1).all().item() for t in outs) and (cols == 0xA5).all().item()
        codec.reserve(n)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            work(codec)                              # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            work(codec)
        torch.cuda.synchronize()
        for b in batches:
            w = np.zeros(wl, np.uint8)
            w[:len(b.wire)] = b.wire
            d_wire[:wl] = torch.from_numpy(w).cuda()
            d_msgs.copy_(torch.from_numpy(b.msgs.view(np.uint8).reshape(-1).copy()).cuda())
            d_st.copy_(torch.from_numpy(b.status.copy()).cuda())
            d_rs.copy_(torch.from_numpy(b.rec_start.view(np.int64).copy()).cuda())
            for t in outs:
                t.fill_(-1)
            cols.fill_(0xA5)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = M.unpack(w, wl, b.msgs, b.status, fields, 0, b.rec_start)
            assert cols.cpu().numpy().tobytes() == M.cols_image(fields, n, cap, want["values"], 0xA5, 32)
            assert xstat.cpu().numpy().view(np.uint32).tolist() == want["xstat"] + [T]
            assert present.cpu().numpy().view(np.uint64).tolist() == want["present"] + [(1 << 64) - 1]
            assert rest_pos.cpu().numpy().view(np.uint32).tolist() == want["rest_pos"] + [T]
            assert rest_len.cpu().numpy().view(np.uint32).tolist() == want["rest_len"] + [T]
            assert res.cpu().numpy().view(np.uint64).tolist() == want["result"] + [(1 << 64) - 1]
    finally:
        fresh.close()
        codec.close()
