"""The host model of onc_payload_slots / onc_place_payloads
(tests/payload_model.py) against independent routes: every placed slice
against the record reassembled by fragment_model and sliced, slot_off against
np.cumsum of the rounded lengths, the fragment-by-fragment form of the copy
against the byte-by-byte loop, and the slices that are not OK."""
import numpy as np
import pytest

import fragment_streams_model as FS
import heads_model as HM
import onc_rpc_amd.layout as L
import payload_model as PM

SENT = 0xA5


def _heads(small=True, order="shuffled"):
    stream, names = PM.place_stream(small=small)
    wire, start, flen = FS.scatter(stream, order, seed=11)
    h = HM.defragment_heads(wire, start, flen, 64)
    records = FS.defragment_extents(wire, start, flen)["records"]
    return wire, start, flen, h, records, names


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_placed_slices_are_slices_of_the_reassembled_records(order):
    wire, start, flen, h, records, names = _heads(order=order)
    pay_pos, pay_len, kinds = PM.choose_slices(h, flen, names)
    assert set(kinds) >= set(PM.KINDS)
    n = len(pay_len)
    for slots, cap in ((PM.pack_slots(pay_len, 1), None), (PM.pack_slots(pay_len, 16), None),
                       (PM.pack_slots(pay_len, 4096), None), PM.odd_slots(pay_len)):
        cap = int(slots[n]) if cap is None else cap
        slow, fast = np.full(cap, SENT, np.uint8), np.full(cap, SENT, np.uint8)
        args = (wire, start, flen, h["rec_frag"], h["frag_pre"], h["rec_len"], pay_pos, pay_len, slots)
        done = PM.place_payloads(*args, slow)
        assert PM.place_payloads_fast(*args, fast) == done and np.array_equal(slow, fast)
        assert done == [r for r in range(n) if pay_len[r]]
        want = np.full(cap, SENT, np.uint8)
        for r in done:                               # the independent route: reassemble, then slice
            p, ln, so = int(pay_pos[r]), int(pay_len[r]), int(slots[r])
            want[so:so + ln] = np.frombuffer(records[r][p:p + ln], np.uint8)
            assert len(records[r][p:p + ln]) == ln
        assert np.array_equal(slow, want)


def test_whole_stream_shapes():
    """The full-size stream of the GPU tests has the shapes they name."""
    stream, names = PM.place_stream()
    wire, start, flen = FS.scatter(stream, "ascending")
    h = HM.defragment_heads(wire, start, flen, 64)
    nf = np.diff(h["rec_frag"].astype(np.int64))
    assert 600 <= int(nf[:150].sum()) <= 900
    assert nf[names["ones"]] > PM.TILE + PM.STAGE and int(h["rec_len"][names["ones"]]) - 4 == nf[names["ones"]]
    assert int(h["rec_len"][names["long"]]) - 4 > 4 * PM.TILE and (flen[int(h["rec_frag"][names["long"]]):] == 4).any()
    pay_pos, pay_len, kinds = PM.choose_slices(h, flen, names)
    run = slice(names["run"], names["run"] + names["run_len"])
    assert names["run_len"] > PM.STAGE and not pay_len[run].any()
    assert pay_len[names["run"] - 1] > 0 and pay_len[names["run"] + names["run_len"]] > 0
    assert int(pay_len[names["long"]]) > 4 * PM.TILE
    # the fast form on the full stream == the independent route
    slots = PM.pack_slots(pay_len, 16)
    got = np.full(int(slots[-1]), SENT, np.uint8)
    PM.place_payloads_fast(wire, start, flen, h["rec_frag"], h["frag_pre"], h["rec_len"], pay_pos, pay_len, slots, got)
    records = FS.defragment_extents(wire, start, flen)["records"]
    for r in np.nonzero(pay_len)[0]:
        p, ln, so = int(pay_pos[r]), int(pay_len[r]), int(slots[r])
        assert got[so:so + ln].tobytes() == records[r][p:p + ln], r


def _descriptors(n, seed=3):
    rng = np.random.default_rng(seed)
    m = np.zeros(n, L.MSG_DTYPE)
    m["msg_type"] = rng.integers(0, 2, n)
    m["reply_stat"] = rng.integers(0, 2, n)
    m["stat"] = rng.integers(0, 3, n)
    m["payload_len"] = rng.choice((0, 1, 15, 16, 17, 4095, 4096, 4097), n)
    m["payload_off"] = np.arange(n) * 160 + rng.integers(24, 160, n)
    status = np.where(rng.random(n) < 0.2, 10, 0).astype(np.int32)
    return m, status


@pytest.mark.parametrize("align", [1, 2, 16, 512, 4096, 1 << 20])
def test_slots_are_the_cumsum_of_the_rounded_lengths(align):
    m, status = _descriptors(500)
    s = PM.payload_slots(m, status, align, head_len=160, want_msgs_out=True)
    has = (status == 0) & (m["payload_len"] > 0) & HM.has_payload(m)
    assert 50 < int(has.sum()) < 450
    lens = np.where(has, m["payload_len"], 0).astype(np.int64)
    rounded = (lens + align - 1) // align * align
    assert np.array_equal(s["slot_off"].astype(np.int64), np.concatenate(([0], np.cumsum(rounded))))
    assert s["result"].tolist() == [int(has.sum()), int(lens.sum()), int(rounded.sum())]
    assert np.array_equal(s["pay_len"], lens) and (s["slot_off"] % align == 0).all()
    pos = np.where(has, m["payload_off"].astype(np.int64) - np.arange(500) * 160, 0)
    assert np.array_equal(s["pay_pos"], pos)
    out = s["msgs_out"]
    assert np.array_equal(out["payload_off"][has], s["slot_off"][:-1][has])
    assert np.array_equal(out["payload_off"][~has], m["payload_off"][~has])
    out["payload_off"] = m["payload_off"]
    assert np.array_equal(out.view(np.uint8), m.view(np.uint8))
    # the rec_start form: the same slots, positions from the extents
    rs = (np.arange(500) * 977 + 13).astype(np.uint64)
    m2 = m.copy()
    m2["payload_off"] = rs + pos.astype(np.uint64) + np.where(has, 0, 5).astype(np.uint64)
    s2 = PM.payload_slots(m2, status, align, rec_start=rs)
    assert np.array_equal(s2["pay_pos"], s["pay_pos"]) and np.array_equal(s2["slot_off"], s["slot_off"])


def test_slices_that_are_not_ok():
    ok = PM.slice_ok
    assert not ok(3, 1, 100, 0, 1000) and ok(4, 1, 100, 0, 1000)
    assert ok(100, 0, 100, 0, 1000) and not ok(100, 1, 100, 0, 1000) and not ok(101, 0, 100, 0, 1000)
    assert ok(4, 96, 100, 0, 1000) and not ok(4, 97, 100, 0, 1000)
    assert not ok(0xFFFFFFFF, 2, 0xFFFFFFFF, 0, 1 << 40)           # pay_pos + pay_len wraps 2^32
    assert not ok(4, 1, 0, 0, 1000)                                 # a record of length 0 (TOO_LONG)
    assert ok(4, 0, 100, 1000, 1000) and not ok(4, 1, 100, 1000, 1000) and not ok(4, 0, 100, 1001, 1000)
    assert ok(4, 10, 100, 990, 1000) and not ok(4, 11, 100, 990, 1000)
    assert not ok(4, 2, 100, (1 << 64) - 1, (1 << 64) - 1)          # slot_off + pay_len wraps 2^64
    # in the copy: nothing is written for them, and empty slices point anywhere
    wire, start, flen, h, records, names = _heads()
    n = len(h["rec_len"])
    pay_pos, pay_len, _ = PM.choose_slices(h, flen, names)
    slots = PM.pack_slots(pay_len, 16)
    good = np.full(int(slots[n]), SENT, np.uint8)
    args = [wire, start, flen, h["rec_frag"], h["frag_pre"], h["rec_len"], pay_pos, pay_len, slots]
    PM.place_payloads(*args, good)
    victims = [r for r in range(2, n - 2) if pay_len[r] >= 2][:3]
    bad_pos, bad_len = pay_pos.copy(), pay_len.copy()
    bad_pos[victims[0]] = 3
    bad_pos[victims[1]] = h["rec_len"][victims[1]] + 1
    bad_len[victims[2]] = h["rec_len"][victims[2]] - pay_pos[victims[2]] + 1
    args[6], args[7] = bad_pos, bad_len
    got = np.full(int(slots[n]), SENT, np.uint8)
    done = PM.place_payloads(*args, got)
    assert not set(victims) & set(done)
    want = good.copy()
    for r in victims:
        want[int(slots[r]):int(slots[r]) + int(pay_len[r])] = SENT
    assert np.array_equal(got, want)
