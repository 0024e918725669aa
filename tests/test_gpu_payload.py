"""Decoded payloads placed in aligned slots on the GPU: onc_payload_slots and
onc_place_payloads (payload.hip) against their host model
(tests/payload_model.py, itself checked on the CPU in
tests/test_payload_model.py), end to end against the payloads of the original
records and the oracle's packed stream, beyond 4 GiB, captured in a graph, and
through the C++ mirror. Every comparison is bit-exact, and every device output
is pre-filled with a sentinel: a stray write fails by comparison. No extent
points outside its buffer.

Two of the slices that are not OK are cut by dst_cap: a slot ending one byte
past it, and slot_off > dst_cap. slot_off is non-decreasing (it is trusted to
be), so nothing with bytes can follow such a record inside dst_cap: these two
stand behind OK neighbours and in front of records without bytes, not between
two OK ones."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fragment_model as FR
import fragment_streams_model as FS
import heads_model as HM
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
import payload_model as PM
import streams_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
GUARD = 64
U32, U64 = 0xFFFFFFFF, np.uint64(2**64 - 1)
INVALID_LENGTH = 10


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codec(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)
    yield c
    c.close()


@pytest.fixture(scope="module")
def messages(oracle):
    """300 random messages as the oracle encodes them: (records, packed wire, offsets)."""
    wire, off, st, _ = oracle.encode_batch(L.build_batch(S.random_messages(300, seed=91, max_payload=1025)))
    assert not st.any()
    return [wire[int(off[i]):int(off[i + 1])] for i in range(300)], wire, off


# ---------------------------------------------------------------------------
# 1. slots
# ---------------------------------------------------------------------------
LENS = (0, 1, 15, 16, 17, 4095, 4096, 4097)


def _slot_descriptors(n=600, head_len=160, seed=5):
    """Descriptor and status arrays as a decode writes them, and as it never
    does: OK Calls and accepted-success replies with every length of LENS;
    denied and non-success replies with a payload_len, non-OK statuses with
    non-zero descriptors (all to be ignored). -> (msgs, status, rec_start,
    each payload's position in its record)."""
    rng = np.random.default_rng(seed)
    m = np.zeros(n, L.MSG_DTYPE)
    m["xid"] = np.arange(n) + 1000
    kind = np.arange(n) % 6          # 0, 1: call; 2: success reply; 3: denied; 4: accepted, not success; 5: call, bad status
    m["msg_type"] = np.where(np.isin(kind, (0, 1, 5)), L.MSG_CALL, L.MSG_REPLY)
    m["reply_stat"] = np.where(kind == 3, L.REPLY_DENIED, L.REPLY_ACCEPTED)
    m["stat"] = np.where(kind == 4, rng.integers(1, 6, n), 0)
    m["payload_len"] = np.array(LENS)[(np.arange(n) // 6) % len(LENS)]
    m["f0"], m["f1"], m["f2"] = 100003, 4, rng.integers(0, 20, n)
    pos = rng.integers(28, head_len, n)
    m["payload_off"] = np.arange(n, dtype=np.uint64) * head_len + pos.astype(np.uint64)
    m["cred_ref"], m["verf_ref"] = rng.integers(0, 1 << 40, n), rng.integers(0, 1 << 40, n)
    status = np.where(kind == 5, rng.choice((1, INVALID_LENGTH, 106), n), 0).astype(np.int32)
    rec_start = (np.arange(n, dtype=np.uint64) * 5000 + rng.integers(0, 900, n).astype(np.uint64) + (1 << 33))
    return m, status, rec_start, pos


def _check_slots(R, codec, m, status, align, head_len, rec_start, out_mode, what):
    want = PM.payload_slots(m, status, align, head_len=head_len, rec_start=rec_start, want_msgs_out=True)
    g = R.payload_slots_host(codec, m, status, align, head_len=head_len, rec_start=rec_start, msgs_out=out_mode)
    n, raw = len(m), g["raw"]
    assert g["result"].tolist() == want["result"].tolist(), f"{what}: result {g['result']} != {want['result']}"
    assert (raw["result"][3:] == U64).all()
    for k in ("pay_pos", "pay_len"):
        assert np.array_equal(raw[k][:n], want[k]), f"{what}: {k}"
        assert (raw[k][n:] == U32).all(), f"{what}: {k} written past n"
    assert np.array_equal(raw["slot_off"][:n + 1], want["slot_off"]), f"{what}: slot_off"
    assert (raw["slot_off"][n + 1:] == U64).all(), f"{what}: slot_off written past n + 1"
    src = m.view(np.uint8).reshape(-1)
    new = want["msgs_out"].view(np.uint8).reshape(-1)
    if out_mode == "inplace":
        assert np.array_equal(raw["msgs"][:64 * n], new), f"{what}: msgs rewritten in place"
    else:
        assert np.array_equal(raw["msgs"][:64 * n], src), f"{what}: msgs changed"
    assert (raw["msgs"][64 * n:] == SENT).all()
    if out_mode == "separate":
        assert np.array_equal(raw["msgs_out"][:64 * n], new), f"{what}: msgs_out"
        assert (raw["msgs_out"][64 * n:] == SENT).all()
    return want


@pytest.mark.parametrize("out_mode", [None, "separate", "inplace"])
@pytest.mark.parametrize("form", ["heads", "rec_start"])
@pytest.mark.parametrize("align", [1, 16, 4096])
def test_slots_against_the_model(R, codec, align, form, out_mode):
    m, status, rec_start, pos = _slot_descriptors()
    if form == "rec_start":
        m = m.copy()
        m["payload_off"] = rec_start + pos.astype(np.uint64)
    rs = rec_start if form == "rec_start" else None
    want = _check_slots(R, codec, m, status, align, 160, rs, out_mode, f"{form} {align} {out_mode}")
    k = int(want["result"][0])
    assert k == int((np.isin(np.arange(600) % 6, (0, 1, 2)) & (m["payload_len"] > 0)).sum()) > 200
    assert set(want["pay_len"].tolist()) == set(LENS)
    assert np.array_equal(want["pay_pos"][want["pay_len"] > 0], pos[want["pay_len"] > 0])
    for n in (0, 1, 2, 256, 257):
        _check_slots(R, codec, m[:n], status[:n], align, 160, None if rs is None else rs[:n], out_mode, f"n = {n}")
    # one record with a payload, and one without
    for i in (0, 3):
        w = _check_slots(R, codec, m[6 + i:7 + i], status[6 + i:7 + i], align, 160,
                         None if rs is None else rs[6 + i:7 + i], out_mode, f"record {6 + i} alone")
        if form == "rec_start":
            assert int(w["result"][0]) == (i == 0)


# ---------------------------------------------------------------------------
# 2. place, fragmented
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def placed_stream():
    """The stream of the fragmented placement tests, scattered three ways, with
    its heads model and the caller's slices: {order: (wire, start, flen, heads
    model, pay_pos, pay_len, names)}."""
    stream, names = PM.place_stream()
    out = {}
    for order in ("ascending", "descending", "shuffled"):
        wire, start, flen = FS.scatter(stream, order, seed=59)
        h = HM.defragment_heads(wire, start, flen, 64)
        pay_pos, pay_len, kinds = PM.choose_slices(h, flen, names)
        assert set(kinds) >= set(PM.KINDS)
        out[order] = (wire, start, flen, h, pay_pos, pay_len, names)
    return out


def _place(R, codec, wire, start, flen, h, pay_pos, pay_len, slots, cap, shift, rec_len=None):
    """onc_place_payloads == the model over dst and GUARD bytes either side."""
    rec_len = h["rec_len"] if rec_len is None else rec_len
    rf, fp = (None, None) if h is None else (h["rec_frag"], h["frag_pre"])
    got = R.place_payloads_host(codec, wire, start, flen, rf, fp, rec_len, pay_pos, pay_len, slots, cap, shift=shift,
                                fill=SENT, guard=GUARD)
    want = np.full(cap, SENT, np.uint8)
    done = PM.place_payloads_fast(wire, start, flen, rf, fp, rec_len, pay_pos, pay_len, slots, want)
    want = np.concatenate((np.full(GUARD, SENT, np.uint8), want, np.full(GUARD, SENT, np.uint8)))
    bad = np.nonzero(got != want)[0]
    if len(bad):
        at = int(bad[0]) - GUARD
        r = int(np.searchsorted(np.asarray(slots[:len(pay_len)], np.uint64), at, side="right")) - 1
        raise AssertionError(f"dst differs first at byte {at} (record {r}, slot {int(slots[r]) if r >= 0 else None}, "
                             f"pay_pos {int(pay_pos[r])}, pay_len {int(pay_len[r])}): {got[bad[:8]]} vs {want[bad[:8]]}; "
                             f"{len(bad)} bytes differ")
    return done


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_place_fragmented_against_the_model(R, codec, placed_stream, order):
    wire, start, flen, h, pay_pos, pay_len, names = placed_stream[order]
    n = len(pay_len)
    assert n > 350 and len(start) > 9000
    lists = [(PM.pack_slots(pay_len, a), None) for a in (1, 16, 4096)] + [PM.odd_slots(pay_len)]
    for k, (slots, cap) in enumerate(lists):
        if cap is None:
            cap = int(slots[n])
        else:                                        # the caller's own list: dst_cap ends with the last slice
            cap = max(int(slots[r]) + int(pay_len[r]) for r in range(n))
        for shift in (0, 1, 5, 15):
            done = _place(R, codec, wire, start, flen, h, pay_pos, pay_len, slots, cap, shift)
            assert done == np.nonzero(pay_len)[0].tolist()
    # slot_off[n] is not read: a list of n entries in a buffer of its own gives the same
    slots = PM.pack_slots(pay_len, 16)
    _place(R, codec, wire, start, flen, h, pay_pos, pay_len, slots[:n], int(slots[n]), 3)
    # a capacity far beyond the slots
    _place(R, codec, wire, start, flen, h, pay_pos, pay_len, slots, int(slots[n]) + 300000, 7)


def test_place_fragmented_in_one_workgroup(R, placed_stream):
    """The same stream with the copy launched as one workgroup
    (ONC_VARIANT_COPY_ONE_GROUP): its slots fill more than four tiles, so
    every wave runs several (tests/test_gpu_tile_runs.py). Against the model,
    as the default launch above."""
    wire, start, flen, h, pay_pos, pay_len, names = placed_stream["shuffled"]
    n = len(pay_len)
    one = R.Codec(0, variant=R.VARIANT_COPY_ONE_GROUP)
    try:
        for slots, cap in [(PM.pack_slots(pay_len, a), None) for a in (1, 4096)] + [PM.odd_slots(pay_len)]:
            cap = int(slots[n]) if cap is None else max(int(slots[r]) + int(pay_len[r]) for r in range(n))
            assert cap > 4 * PM.TILE
            for shift in (0, 15):
                done = _place(R, one, wire, start, flen, h, pay_pos, pay_len, slots, cap, shift)
                assert done == np.nonzero(pay_len)[0].tolist()
        # cut by dst_cap in the middle of the long record's slot, and of a tile
        slots = PM.pack_slots(pay_len, 16)
        cap = int(slots[names["long"]]) + 2 * PM.TILE + 1000
        done = _place(R, one, wire, start, flen, h, pay_pos, pay_len, slots, cap, 9)
        assert done == [r for r in np.nonzero(pay_len)[0].tolist() if r < names["long"]]
    finally:
        one.close()


# ---------------------------------------------------------------------------
# 3. slices that are not OK
# ---------------------------------------------------------------------------
def test_slices_that_are_not_ok_are_left_alone(R, codec, placed_stream):
    wire, start, flen, h, pay_pos, pay_len, names = placed_stream["shuffled"]
    n = len(pay_len)
    rec_len = h["rec_len"].copy()
    pos, ln = pay_pos.copy(), pay_len.copy()
    whole = [r for r in range(3, names["ones"] - 3) if ln[r] >= 2 and ln[r - 1] and ln[r + 1]][::3][:5]
    assert len(whole) == 5 and all(b - a > 1 for a, b in zip(whole, whole[1:]))
    v = dict(zip(("pos3", "past_end", "too_long", "wraps", "rec_len0"), whole))
    pos[v["pos3"]] = 3
    pos[v["past_end"]], ln[v["past_end"]] = rec_len[v["past_end"]] + 1, 1
    ln[v["too_long"]] = rec_len[v["too_long"]] - pos[v["too_long"]] + 1
    # pay_pos <= rec_len, and the sum wraps to 0x10: inside the record, were it formed
    pos[v["wraps"]], ln[v["wraps"]], rec_len[v["wraps"]] = 0xFFFFFFF0, 0x20, 0xFFFFFFFF
    rec_len[v["rec_len0"]] = 0                                   # ONC_ENC_TOO_LONG
    for align, shift in ((1, 0), (16, 9), (4096, 15)):
        # the slots are the caller's, sized by what it meant to place
        slots = PM.pack_slots(np.maximum(ln, pay_len), align)
        done = _place(R, codec, wire, start, flen, h, pos, ln, slots, int(slots[n]), shift, rec_len=rec_len)
        assert not set(whole) & set(done)
        assert all(r - 1 in done and r + 1 in done for r in whole)
    # cut by dst_cap: the last records with bytes, behind OK neighbours
    last = [int(r) for r in np.nonzero(pay_len)[0][-3:]]
    slots = PM.pack_slots(pay_len, 16)
    slots[last[2]:] += np.uint64(16)                             # (a gap in front of the last slot)
    end = int(slots[last[2]]) + int(pay_len[last[2]])
    for cap, gone in ((end, []), (end - 1, last[2:]), (int(slots[last[2]]), last[2:]), (int(slots[last[2]]) - 1, last[2:]),
                      (int(slots[last[1]]) + int(pay_len[last[1]]) - 1, last[1:]), (0, None)):
        for shift in (0, 11):
            done = _place(R, codec, wire, start, flen, h, pay_pos, pay_len, slots, cap, shift)
            if gone is not None:
                assert done == [int(r) for r in np.nonzero(pay_len)[0] if r not in gone]
            else:
                assert done == []


# ---------------------------------------------------------------------------
# 4, 5. end to end
# ---------------------------------------------------------------------------
def _dev(arr, dtype, view, extra=1):
    import torch
    a = np.ascontiguousarray(arr, dtype)
    return torch.from_numpy(np.append(a, np.zeros(extra, dtype)).view(view).copy()).cuda()


def _slots_place_reencode(R, codec, bufs, n, recs, packed, packed_off, align, d_wire, d_fs, d_fl, nfrag, d_rf, d_fp,
                          d_rl, auth_arena, auth_len, host_src, head_len=0, d_rs=None, what=""):
    """onc_payload_slots (msgs_out) -> onc_place_payloads -> onc_encode of the
    decoded batch `bufs`, all on the device. host_src: (wire, start, flen,
    heads model or None, rec_len, base of record r's offsets) for the model."""
    import torch
    wire, start, flen, h, rec_len, base = host_src
    pay_pos = torch.full((n + 4,), -1, dtype=torch.int32, device="cuda")
    pay_len = torch.full((n + 4,), -1, dtype=torch.int32, device="cuda")
    slot_off = torch.full((n + 5,), -1, dtype=torch.int64, device="cuda")
    res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    msgs_out = torch.full(((n + 1) * 64,), SENT, dtype=torch.uint8, device="cuda")
    codec.payload_slots(bufs.msgs, bufs.status, n, align, pay_pos, pay_len, slot_off, res, head_len=head_len,
                        rec_start=d_rs, msgs_out=msgs_out)
    codec.sync()
    gm, gu, gs, _, _ = bufs.to_host()
    assert not gs.any(), f"{what}: every record decodes"
    want = PM.payload_slots(gm, gs, align, head_len=head_len, rec_start=base if d_rs is not None else None,
                            want_msgs_out=True)
    r3 = res.cpu().numpy().view(np.uint64)
    assert r3.tolist() == want["result"].tolist()
    g_pos, g_len = pay_pos.cpu().numpy().view(np.uint32), pay_len.cpu().numpy().view(np.uint32)
    g_off = slot_off.cpu().numpy().view(np.uint64)
    assert np.array_equal(g_pos[:n], want["pay_pos"]) and np.array_equal(g_len[:n], want["pay_len"])
    assert np.array_equal(g_off[:n + 1], want["slot_off"]) and (g_off[n + 1:] == U64).all() and (g_pos[n:] == U32).all()
    assert np.array_equal(msgs_out.cpu().numpy()[:64 * n], want["msgs_out"].view(np.uint8).reshape(-1))
    cap = int(r3[2])
    dbase, lo = R.aligned_bytes(GUARD + cap + GUARD, SENT, "cuda")
    dst = dbase[lo + GUARD:lo + GUARD + cap + GUARD]
    codec.place_payloads(d_wire, d_fs, d_fl, nfrag, d_rf, d_fp, d_rl, pay_pos, pay_len, slot_off, n, dst, dst_cap=cap)
    codec.sync()
    got = dbase.cpu().numpy()[lo:lo + GUARD + cap + GUARD]
    model = np.full(cap, SENT, np.uint8)
    rf, fp = (None, None) if h is None else (h["rec_frag"], h["frag_pre"])
    PM.place_payloads_fast(wire, start, flen, rf, fp, rec_len, want["pay_pos"], want["pay_len"], want["slot_off"], model)
    assert np.array_equal(got[GUARD:GUARD + cap], model), f"{what}: placed bytes != the model"
    assert (got[:GUARD] == SENT).all() and (got[GUARD + cap:] == SENT).all()
    # every OK record's placed bytes are the payload in the original record
    checked = 0
    for i in np.nonzero(want["pay_len"])[0]:
        p, ln, so = int(want["pay_pos"][i]), int(want["pay_len"][i]), int(want["slot_off"][i])
        assert p + ln == len(recs[i]) and so % align == 0
        assert got[GUARD + so:GUARD + so + ln].tobytes() == recs[i][p:], i
        checked += 1
    assert checked == int(r3[0]) > 40
    # the decoded batch re-encodes from the heads (or the wire) and the placed buffer
    db = R.DeviceBatch(n, msgs_out, bufs.unix, auth_arena, dst, unix_count=2 * n, auth_len=auth_len, payload_len=cap)
    total = len(packed)
    out = torch.full((total + 64,), SENT, dtype=torch.uint8, device="cuda")
    rec_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    codec.encode(db, out, rec_off, status, None, out_cap=total)
    codec.sync()
    assert not status.cpu().numpy().any()
    assert np.array_equal(rec_off.cpu().numpy().view(np.uint64), packed_off)
    o = out.cpu().numpy()
    assert o[:total].tobytes() == packed and (o[total:] == SENT).all(), f"{what}: the re-encode differs from the oracle's stream"


def test_end_to_end_fragmented(R, codec, messages):
    import torch
    from test_gpu_heads import _fragmented_slab
    recs, packed, packed_off = messages
    n, head_len = 300, 736
    slab, off, ln = _fragmented_slab(recs, 93)
    start, flen, _, rows, fres = R.frame_host_fragment_streams(codec, slab, off, ln, with_seg=False)
    assert int(fres[2]) == n and int(fres[0]) > 3000 and (rows[:, 3] == 0).all()
    nfrag = len(start)
    g = R.defragment_host_heads(codec, slab, start, flen, head_len, max_records=n, fill=0)
    h = HM.defragment_heads(slab, start, flen, head_len)
    assert g["result"].tolist() == h["result"].tolist() and g["rec_len"].tolist() == [len(r) for r in recs]
    hbase, lo = R.aligned_bytes(n * head_len, 0, "cuda")
    hbase[lo:lo + n * head_len] = torch.from_numpy(g["heads"][:n * head_len].copy()).cuda()
    heads = hbase[lo:lo + n * head_len]
    d_rl = _dev(g["rec_len"], np.uint32, np.int32)
    bufs = R.DecodeBuffers(n)
    codec.decode_heads(heads, head_len, d_rl, n, L.DECODE_SLICE, bufs.msgs, bufs.unix, bufs.status, bufs.aux0, bufs.aux1)
    d_wire = R.to_device(np.frombuffer(slab + b"\0" * 16, np.uint8), "cuda")
    d_fs, d_fl = _dev(start, np.uint64, np.int64), _dev(flen, np.uint32, np.int32)
    d_rf, d_fp = _dev(g["rec_frag"], np.uint64, np.int64), _dev(g["frag_pre"], np.uint64, np.int64)
    for align in (1, 16, 512):
        _slots_place_reencode(R, codec, bufs, n, recs, packed, packed_off, align, d_wire, d_fs, d_fl, nfrag, d_rf, d_fp,
                              d_rl, heads, n * head_len, (slab, start, flen, h, h["rec_len"], None),
                              head_len=head_len, what=f"fragmented, align {align}")


def test_end_to_end_single_fragment(R, codec, messages):
    recs, packed, packed_off = messages
    n = 300
    rng = np.random.default_rng(94)
    sl = SM.Slab(front=int(rng.integers(0, 16)))
    cut = np.sort(rng.integers(0, n + 1, 19)).tolist()
    for a, b in zip([0] + cut, cut + [n]):
        sl.add(b"".join(recs[a:b]), gap=int(rng.integers(0, 24)))
    slab, off, ln = sl.done()
    rec_start, rec_len, _, rows, res = R.frame_host_streams(codec, slab, off, ln, with_seg=False)
    assert int(res[0]) == n and rec_len.tolist() == [len(r) for r in recs]
    d_wire = R.to_device(np.frombuffer(slab + b"\0" * 16, np.uint8), "cuda")
    d_rs, d_rl = _dev(rec_start, np.uint64, np.int64), _dev(rec_len, np.uint32, np.int32)
    bufs = R.DecodeBuffers(n)
    codec.decode_extents(d_wire, len(slab), d_rs, d_rl, n, L.DECODE_SLICE, bufs.msgs, bufs.unix, bufs.status, bufs.aux0,
                         bufs.aux1)
    for align in (1, 16, 512):
        # the identity form: record r is fragment r
        _slots_place_reencode(R, codec, bufs, n, recs, packed, packed_off, align, d_wire, d_rs, d_rl, n, None, None, d_rl,
                              d_wire, len(slab), (slab, rec_start, rec_len, None, rec_len, rec_start), d_rs=d_rs,
                              what=f"single fragment, align {align}")


# ---------------------------------------------------------------------------
# 6. beyond 4 GiB
# ---------------------------------------------------------------------------
def test_beyond_4gib(R, codec):
    """Fragments below, across and above wire byte 2^32, placed in slots below,
    across and above dst byte 2^32: every index is 64 bits wide."""
    import torch
    G = 1 << 32
    size = G + (1 << 20)
    rng = np.random.default_rng(77)
    # (fragment start, body bytes, last); record 0: one fragment; record 1: three, the middle one across 2^32
    frags = [(1000, 4000, True), (G - 6000, 3000, False), (G - 1500, 3000, False), (G + 100000, 2000, True),
             (G + 500000, 5000, True)]
    bodies = [rng.bytes(b) for _, b, _ in frags]
    wire = torch.empty(size, dtype=torch.uint8, device="cuda")           # allocated, never filled
    for (at, b, last), body in zip(frags, bodies):
        raw = FR._BE.pack((FR.LAST if last else 0) | b) + body
        wire[at:at + len(raw)] = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
    start = np.array([f[0] for f in frags], np.uint64)
    flen = np.array([f[1] + 4 for f in frags], np.uint32)
    rec_frag = np.array([0, 1, 4, 5], np.uint64)
    frag_pre = np.array([0, 0, 3000, 6000, 0], np.uint64)
    payloads = [bodies[0], bodies[1] + bodies[2] + bodies[3], bodies[4]]
    rec_len = np.array([len(p) + 4 for p in payloads], np.uint32)
    # the caller's slices: the whole of records 0 and 2, record 1 from inside its first fragment to inside its last
    pay_pos = np.array([4, 4 + 100, 4], np.uint32)
    pay_len = np.array([4000, 7800, 5000], np.uint32)
    want = [payloads[0], payloads[1][100:7900], payloads[2]]
    slots = np.array([100, G - 4003, G + 300001], np.uint64)             # below, across and above 2^32, at odd addresses
    dst = torch.empty(size, dtype=torch.uint8, device="cuda")
    win = [(max(0, int(s) - 4096), int(s) + int(n) + 4096) for s, n in zip(slots, pay_len)]
    for a, b in win:
        dst[a:b] = SENT
    d = [_dev(x, t, v) for x, t, v in ((start, np.uint64, np.int64), (flen, np.uint32, np.int32),
                                       (rec_frag, np.uint64, np.int64), (frag_pre, np.uint64, np.int64),
                                       (rec_len, np.uint32, np.int32), (pay_pos, np.uint32, np.int32),
                                       (pay_len, np.uint32, np.int32), (slots, np.uint64, np.int64))]
    codec.place_payloads(wire, d[0], d[1], len(frags), d[2], d[3], d[4], d[5], d[6], d[7], 3, dst, dst_cap=size)
    codec.sync()
    for (a, b), s, w in zip(win, slots, want):
        got = dst[a:b].cpu().numpy()
        exp = np.full(b - a, SENT, np.uint8)
        exp[int(s) - a:int(s) - a + len(w)] = np.frombuffer(w, np.uint8)
        bad = np.nonzero(got != exp)[0]
        assert len(bad) == 0, f"slot {int(s)}: differs first at dst byte {a + int(bad[0])}"
    # a capacity that cuts the slot across 2^32 and the one above it
    for a, b in win:
        dst[a:b] = SENT
    codec.place_payloads(wire, d[0], d[1], len(frags), d[2], d[3], d[4], d[5], d[6], d[7], 3, dst, dst_cap=G + 3796)
    codec.sync()
    for k, ((a, b), s, w) in enumerate(zip(win, slots, want)):
        got = dst[a:b].cpu().numpy()
        exp = np.full(b - a, SENT, np.uint8)
        if k == 0:
            exp[int(s) - a:int(s) - a + len(w)] = np.frombuffer(w, np.uint8)
        assert np.array_equal(got, exp), k


# ---------------------------------------------------------------------------
# 7. graph capture
# ---------------------------------------------------------------------------
def _synth_msgs(pay_pos, pay_len, head_len, n_pad):
    """Call descriptors whose payload is the slice: what a decode of records
    with those payloads writes, as far as onc_payload_slots reads it. Records
    from len(pay_pos) to n_pad failed their decode."""
    n = len(pay_pos)
    m = np.zeros(n_pad, L.MSG_DTYPE)
    m["msg_type"] = L.MSG_CALL
    m["payload_len"][:n] = pay_len
    m["payload_off"][:n] = np.arange(n, dtype=np.uint64) * head_len + pay_pos
    m["payload_len"][n:], m["payload_off"][n:] = 77, 5
    status = np.zeros(n_pad, np.int32)
    status[n:] = INVALID_LENGTH
    return m, status


def test_graph_capture_and_replay(R):
    import torch
    head_len, align = 64, 16
    inputs = []
    for seed in (81, 82):
        stream, names = PM.place_stream(seed=seed, small=True)
        wire, start, flen = FS.scatter(stream, "shuffled", seed=seed)
        h = HM.defragment_heads(wire, start, flen, head_len)
        pay_pos, pay_len, _ = PM.choose_slices(h, flen, names, seed=seed)
        inputs.append((wire, start, flen, h, pay_pos, pay_len))
    n = max(len(x[5]) for x in inputs) + 3
    nfrag = max(len(x[1]) for x in inputs)
    wsize = max(len(x[0]) for x in inputs) + 16
    cap = max(int(PM.pack_slots(x[5], align)[-1]) for x in inputs) + 256
    d_wire = torch.zeros(wsize, dtype=torch.uint8, device="cuda")
    d_fs = torch.zeros(nfrag + 1, dtype=torch.int64, device="cuda")
    d_fl = torch.full((nfrag + 1,), 4, dtype=torch.int32, device="cuda")
    d_rf = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_fp = torch.zeros(nfrag + 1, dtype=torch.int64, device="cuda")
    d_rl = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_msgs = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    pay_pos = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    pay_len = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    slot_off = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    dst = torch.full((cap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def work(codec):
        codec.payload_slots(d_msgs, d_st, n, align, pay_pos, pay_len, slot_off, res, head_len=head_len)
        codec.place_payloads(d_wire, d_fs, d_fl, nfrag, d_rf, d_fp, d_rl, pay_pos, pay_len, slot_off, n, dst, dst_cap=cap)

    def put(t, a):
        t[:a.size] = torch.from_numpy(a.copy()).cuda()

    fresh = R.Codec(0, stream=s.cuda_stream)
    codec = R.Codec(0, stream=s.cuda_stream)
    try:
        # without the reserve, the slots would grow their scratch inside the capture
        err = None
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            try:
                fresh.payload_slots(d_msgs, d_st, n, align, pay_pos, pay_len, slot_off, res, head_len=head_len)
            except R.CodecError as e:
                err = str(e)
        assert err is not None and "rc=-5" in err, err
        codec.reserve(n)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            work(codec)                              # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            work(codec)
        torch.cuda.synchronize()
        for wire, start, flen, h, p_pos, p_len in inputs:
            k = len(p_len)
            m, st = _synth_msgs(p_pos, p_len, head_len, n)
            rec_frag = np.full(n + 1, len(start), np.uint64)     # the records past k have no fragments
            rec_frag[:k + 1] = h["rec_frag"]
            rec_len = np.zeros(n, np.uint32)
            rec_len[:k] = h["rec_len"]
            d_wire.zero_()
            put(d_wire, np.frombuffer(wire, np.uint8))
            put(d_fs, start.view(np.int64))
            put(d_fl, flen.view(np.int32))
            put(d_rf, rec_frag.view(np.int64))
            put(d_fp, h["frag_pre"].view(np.int64))
            put(d_rl, rec_len.view(np.int32))
            put(d_msgs, m.view(np.uint8).reshape(-1))
            put(d_st, st)
            dst.fill_(SENT)
            g.replay()
            torch.cuda.synchronize()
            want = PM.payload_slots(m, st, align, head_len=head_len)
            assert res.cpu().numpy().view(np.uint64).tolist() == want["result"].tolist()
            assert np.array_equal(slot_off.cpu().numpy().view(np.uint64)[:n + 1], want["slot_off"])
            assert np.array_equal(pay_pos.cpu().numpy().view(np.uint32)[:n], want["pay_pos"])
            assert np.array_equal(pay_len.cpu().numpy().view(np.uint32)[:n], want["pay_len"])
            assert np.array_equal(want["pay_len"][:k], p_len) and np.array_equal(want["pay_pos"][:k][p_len > 0], p_pos[p_len > 0])
            exp = np.full(cap + GUARD, SENT, np.uint8)
            PM.place_payloads_fast(wire, start, flen, rec_frag, h["frag_pre"], rec_len, want["pay_pos"], want["pay_len"],
                                   want["slot_off"], exp[:cap])
            assert np.array_equal(dst.cpu().numpy(), exp)
    finally:
        fresh.close()
        codec.close()


# ---------------------------------------------------------------------------
# 8. the C++ mirror
# ---------------------------------------------------------------------------
def _fnv1a(b):
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


@pytest.mark.parametrize("align", [16, 4096])
def test_cpp_mirror_place_payloads(oracle, messages, tmp_path, align):
    """FragmentedHeads::place_payloads and place_payloads (include/onc_rpc.hpp)
    on a fragmented slab written here: tests/cpp_payload/test_payload.cpp
    compares every placed payload with the one gathered on the host and prints
    its hash, which is the hash of the payload in the original record."""
    exe = os.path.join(ROOT, "tests", "cpp_payload", "test_payload")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    recs = messages[0][:120]
    rng = np.random.default_rng(95)
    sl = SM.Slab(front=3)
    cut = np.sort(rng.integers(0, len(recs) + 1, 11)).tolist()
    plain = 0
    for s, (lo, hi) in enumerate(zip([0] + cut, cut + [len(recs)])):
        data = b""
        for rec in recs[lo:hi]:
            mf = int(rng.integers(8, 200))
            data += rec if s % 3 == 0 else FR.fragment(rec[4:], list(range(mf, len(rec) - 4, mf)))
        if s % 4 == 1:
            data += FR._BE.pack(12) + b"pending run."
        plain += hi - lo if s % 3 == 0 else 0
        sl.add(data, gap=int(rng.integers(0, 24)))
    slab, off, ln = sl.done()
    src, dst = str(tmp_path / "slab.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<QQ", len(off), len(slab)) + off.tobytes() + ln.tobytes() + slab)
    r = subprocess.run([exe, src, dst, str(align)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and "PASS test_payload" in r.stdout, r.stdout + r.stderr
    out = open(dst, "rb").read()
    n_rec, n_pay, pay_bytes, cap, placed_plain = struct.unpack_from("<QQQQQ", out)
    rec_t = np.dtype([("st", "<i4"), ("xid", "<u4"), ("plen", "<u4"), ("fnv", "<u4"), ("slot", "<u8")])
    assert n_rec == len(recs) and 40 + rec_t.itemsize * n_rec == len(out)
    got = np.frombuffer(out, rec_t, n_rec, 40)
    wire = np.frombuffer(b"".join(recs) + b"\0" * 16, np.uint8).copy()
    o = np.concatenate(([0], np.cumsum([len(x) for x in recs]))).astype(np.uint64)
    om, _, ost, _, _ = oracle.decode_batch(wire, o, L.DECODE_SLICE)
    assert not ost.any() and not got["st"].any()
    has = HM.has_payload(om) & (om["payload_len"] > 0)
    plen = np.where(has, om["payload_len"], 0)
    assert np.array_equal(got["xid"], om["xid"]) and np.array_equal(got["plen"], plen)
    w = wire.tobytes()
    assert got["fnv"].tolist() == [_fnv1a(w[int(a):int(a) + int(b)]) for a, b in zip(om["payload_off"], plen)]
    rounded = (plen.astype(np.int64) + align - 1) // align * align
    assert np.array_equal(got["slot"].astype(np.int64), np.cumsum(rounded) - rounded)
    assert [n_pay, pay_bytes, cap] == [int(has.sum()), int(plen.sum()), int(rounded.sum())] and n_pay > 40
    # the segments that do not fragment are decoded in place; those records that carry a payload are placed
    assert 0 < placed_plain <= plain
