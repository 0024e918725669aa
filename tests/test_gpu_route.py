"""Decoded Calls dispatched to handlers on the GPU: onc_route_calls
(route.hip) against its host model (tests/route_model.py, itself checked on
the CPU in tests/test_route_model.py). Every output array is compared whole
and bit-exactly, with the optional outputs given and not given, and every
device output is pre-filled with a sentinel with guard words behind it: a
stray write fails by comparison. Every input is one the interface defines a
result for."""
import os
import struct
import subprocess

import numpy as np
import pytest

import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
import route_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
U32, U64 = 0xFFFFFFFF, np.uint64(2**64 - 1)
H31, TOP = 0x80000000, 0xFFFFFFFF


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


def _check(R, codec, msgs, status, tab, nh, what, want=None):
    """onc_route_calls with and without the optional outputs against the model -> the model's result."""
    want = M.route_calls(msgs, status, tab, nh) if want is None else want
    n = len(msgs)
    for calls_out, replies in ((True, True), (False, False), (True, False), (False, True)):
        g = R.route_calls_host(codec, msgs, status, tab, nh, calls_out=calls_out, replies=replies)
        raw, w = g["raw"], f"{what} (calls_out {calls_out}, replies {replies})"
        assert g["result"].tolist() == want["result"].tolist(), f"{w}: result {g['result']} != {want['result']}"
        assert (raw["result"][4:] == U64).all(), f"{w}: result written past 4"
        assert np.array_equal(g["bin_first"], want["bin_first"]), f"{w}: bin_first"
        assert (raw["bin_first"][nh + 4:] == U64).all(), f"{w}: bin_first written past nh + 4"
        bad = want["route"] is None
        for k in ("route", "order"):
            if bad:
                assert (raw[k] == U32).all(), f"{w}: {k} written for a bad table"
            else:
                assert np.array_equal(g[k], want[k]), f"{w}: {k}"
                assert (raw[k][n:] == U32).all(), f"{w}: {k} written past n"
        for k, on in (("calls_out", calls_out), ("replies", replies)):
            if not on:
                assert g[k] is None
            elif bad:
                assert (raw[k] == SENT).all(), f"{w}: {k} written for a bad table"
            else:
                assert g[k].tobytes() == want[k].tobytes(), f"{w}: {k}"
                assert (raw[k][64 * n:] == SENT).all(), f"{w}: {k} written past n"
        if not bad and n:
            # stability, directly: order is strictly increasing inside each bin
            o, first = g["order"].astype(np.int64), g["bin_first"].astype(np.int64)
            inside = np.ones(n, bool)
            inside[first[(first > 0) & (first < n)]] = False
            assert (np.diff(o)[inside[1:]] > 0).all(), f"{w}: order not ascending inside a bin"
            assert np.array_equal(np.sort(o), np.arange(n)), f"{w}: order is no permutation"
    return want


def make_table(nh, ntab):
    """A valid table of ntab entries over nh handlers -> (rows, a key for every handler it reaches)."""
    rows, key_of = [], {}
    if ntab == 0:
        return rows, key_of
    assert nh >= 1
    cut = np.linspace(0, nh, ntab + 1).astype(int)
    for i in range(ntab):
        prog, ver, pf = 100 + i // 4, 1 + (i // 2) % 2, 1000 * (i % 2)
        if ntab <= nh:                               # the handlers dealt out in runs, a procedure each
            rows.append((prog, ver, pf, int(cut[i + 1] - cut[i]), int(cut[i]), 0))
            for h in range(cut[i], cut[i + 1]):
                key_of[h] = (prog, ver, pf + h - int(cut[i]))
        else:                                        # more entries than handlers: a range for one handler
            rows.append((prog, ver, pf, 1 + i % 3, i % nh, M.ONE_HANDLER))
            key_of.setdefault(i % nh, (prog, ver, pf + i % 3))
    return rows, key_of


def records_for(bins, nh, key_of, seed=0):
    """Descriptors and statuses that the model sends to `bins`: handler bins
    through key_of, rejected ones through keys no entry serves (of every
    kind), not-a-Call as msg_type 1 and 7, failed as random bytes."""
    rng = np.random.default_rng(seed)
    n = len(bins)
    m = np.zeros(n, L.MSG_DTYPE)
    status = np.zeros(n, np.int32)
    m["xid"] = rng.integers(0, 1 << 32, n)
    m["payload_len"], m["payload_off"] = rng.integers(0, 1 << 32, n), rng.integers(0, 1 << 63, n)
    m["cred_ref"], m["verf_kind_len"] = rng.integers(0, 1 << 40, n), rng.integers(0, 1 << 32, n)
    miss = [(7, 7, 7), (100, 9, 0), (100, 1, 999), (100, 1, 5000), (99, 1, 0), (TOP, TOP, TOP)]
    for r, b in enumerate(bins):
        if b < nh:
            m[r]["f0"], m[r]["f1"], m[r]["f2"] = key_of[b]
        elif b == nh:
            m[r]["f0"], m[r]["f1"], m[r]["f2"] = miss[r % len(miss)]
        elif b == nh + 1:
            m[r]["msg_type"] = (L.MSG_REPLY, 7)[r % 2]
        else:
            m[r] = np.frombuffer(rng.bytes(64), L.MSG_DTYPE)[0]
            status[r] = (1, 10, 106, -3)[r % 4]
    return m, status


def reachable(nh, key_of):
    return np.array(sorted(key_of) + [nh, nh + 1, nh + 2])


T = 1024
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1)
SHAPES = [(nh, ntab) for nh in (0, 1, 2, 253) for ntab in (0, 1, 2, 1024) if nh or not ntab]


def test_tile_constant(R):
    assert R.ROUTE_TILE == T


def test_no_records_on_a_fresh_handle(R):
    """The first call of a handle, with no records: the bins' totals are still
    scanned, so the scratch has to be there for them."""
    rows, _ = make_table(5, 3)
    m, status = records_for(np.zeros(0, int), 5, {})
    fresh = R.Codec(0)
    try:
        want = _check(R, fresh, m, status, M.table(rows), 5, "fresh handle, n 0")
        assert want["result"].tolist() == [0, 0, 0, 0] and not want["bin_first"].any()
    finally:
        fresh.close()


@pytest.mark.parametrize("nh,ntab", SHAPES)
def test_sizes(R, codec, nh, ntab):
    rows, key_of = make_table(nh, ntab)
    tab = M.table(rows)
    assert M.first_bad(tab, nh) == 0 and len(tab) == ntab
    reach = reachable(nh, key_of)
    rng = np.random.default_rng(nh * 2000 + ntab)
    for n in SIZES:
        bins = reach[rng.integers(0, len(reach), n)]
        m, status = records_for(bins, nh, key_of, seed=n)
        want = _check(R, codec, m, status, tab, nh, f"nh {nh} ntab {ntab} n {n}")
        assert np.array_equal(want["route"], bins)


@pytest.mark.parametrize("nh", (2, 253))
def test_distributions(R, codec, nh):
    rows, key_of = make_table(nh, min(nh, 60))
    tab = M.table(rows)
    n, nb = 3 * T + 1, nh + 3
    r = np.arange(n)
    cases = {
        "all in handler 0": np.zeros(n, int),
        "all in the last handler": np.full(n, nh - 1),
        "all rejected": np.full(n, nh),
        "all failed": np.full(n, nh + 2),
        "cycling": r % nb,
        "descending blocks": nb - 1 - r * nb // n,
        "one of the highest bin, then bin 0": np.where(r == 0, nb - 1, 0),
        "two bins alternating": np.where(r % 2 == 0, nh + 2, 0),
        "two neighbours alternating": np.where(r % 2 == 0, nh, nh - 1),
    }
    for name, bins in cases.items():
        m, status = records_for(bins, nh, key_of, seed=len(name))
        want = _check(R, codec, m, status, tab, nh, f"nh {nh}: {name}")
        assert np.array_equal(want["route"], bins)
    want = M.route_calls(*records_for(cases["descending blocks"], nh, key_of), tab, nh)
    assert want["order"][0] > want["order"][-1]          # (the blocks come out reversed)


def test_outcomes(R, codec):
    nh = 12
    rows = [(200, 2, 0, 4, 0, 0), (200, 3, 0, 4, 0, 0), (200, 7, 0, 2, 4, 1),                # versions {2, 3, 7}
            (300, 5, 0, 3, 6, 0), (300, 5, 6, 2, 9, 1), (300, 5, 8, 1, 11, 0),               # a gap at 3..5
            (H31, H31, H31, 2, 0, 0), (TOP, TOP, TOP - 2, 2, 2, 1), (TOP, TOP, TOP, 1, 3, 0)]   # ... ends at 2^32
    tab = M.table(rows)
    assert M.first_bad(tab, nh) == 0
    keys = [(200, 1, 0), (200, 4, 1), (200, 8, 0), (200, 2, 3), (200, 2, 4), (200, 7, 1), (200, 7, 2), (200, 0, 0),
            (300, 5, 2), (300, 5, 3), (300, 5, 4), (300, 5, 5), (300, 5, 6), (300, 5, 7), (300, 5, 8), (300, 5, 9),
            (300, 4, 0), (300, 6, 0), (299, 5, 0), (301, 5, 0), (0, 0, 0),
            (H31, H31, H31), (H31, H31, H31 + 1), (H31, H31, H31 + 2), (H31, H31, H31 - 1), (H31, H31 - 1, H31),
            (H31 - 1, H31, H31), (H31 + 1, H31, H31), (TOP, TOP, TOP), (TOP, TOP, TOP - 1), (TOP, TOP, TOP - 2),
            (TOP, TOP, TOP - 3), (TOP, TOP - 1, TOP), (TOP - 1, TOP, TOP), (TOP, 0, 0), (H31, TOP, 0)]
    m = M.calls(keys * 3, xid0=0xFFFFFFF0)
    want = _check(R, codec, m, np.zeros(len(m), np.int32), tab, nh, "outcomes")
    got = {k: (int(want["route"][i]), int(want["stat"][i])) for i, k in enumerate(keys)}
    rep = {int(x["xid"]): x for x in want["replies"]}
    for i, k in enumerate(keys[:3]):                          # versions 1, 4, 8 of {2, 3, 7}
        assert got[k] == (nh, M.PROG_MISMATCH)
        x = rep[(0xFFFFFFF0 + i) & U32]
        assert (int(x["f0"]), int(x["f1"]), int(x["f2"])) == (2, 7, 0)
    assert got[(200, 2, 3)] == (3, 0) and got[(200, 2, 4)] == (nh, M.PROC_UNAVAIL)
    assert got[(200, 7, 1)] == (4, 0) and got[(200, 7, 2)] == (nh, M.PROC_UNAVAIL)
    assert [got[(300, 5, c)][0] for c in range(2, 10)] == [8, nh, nh, nh, 9, 9, 11, nh]      # both edges of the gap
    assert got[(299, 5, 0)] == (nh, M.PROG_UNAVAIL) and got[(0, 0, 0)] == (nh, M.PROG_UNAVAIL)
    assert got[(H31, H31, H31 + 1)] == (1, 0) and got[(H31, H31, H31 + 2)] == (nh, M.PROC_UNAVAIL)
    assert got[(H31, H31 - 1, H31)] == (nh, M.PROG_MISMATCH) and got[(H31 - 1, H31, H31)] == (nh, M.PROG_UNAVAIL)
    assert got[(TOP, TOP, TOP)] == (3, 0) and got[(TOP, TOP, TOP - 1)] == (2, 0) and got[(TOP, TOP, TOP - 2)] == (2, 0)
    assert got[(TOP, TOP, TOP - 3)] == (nh, M.PROC_UNAVAIL) and got[(TOP, 0, 0)] == (nh, M.PROG_MISMATCH)


def test_not_looked_at_and_pass_through(R, codec):
    nh = 3
    tab = M.table([(100003, 3, 0, 3, 0, 0)])
    rng = np.random.default_rng(17)
    n = 200
    m = np.frombuffer(rng.bytes(64 * n), L.MSG_DTYPE).copy()
    status = np.array([(1, 2, 10, 106, -1)[i % 5] for i in range(n)], np.int32)
    kind = np.arange(n) % 4
    # 1: OK records that are no Calls, with msg_type 1 and 7; 2, 3: OK Calls with random other words
    status[kind != 0] = 0
    m["msg_type"][kind == 1] = np.where(np.arange(n)[kind == 1] % 8 == 1, 1, 7)
    m["msg_type"][kind >= 2] = L.MSG_CALL
    m["f0"][kind >= 2], m["f1"][kind >= 2] = 100003, 3
    m["f2"][kind == 2] = rng.integers(0, 3, (kind == 2).sum())
    m["payload_off"][kind == 2] = (1 << 32) + rng.integers(1, 1 << 40, (kind == 2).sum()).astype(np.uint64)
    want = _check(R, codec, m, status, tab, nh, "not looked at")
    assert (want["route"][kind == 0] == nh + 2).all() and (want["route"][kind == 1] == nh + 1).all()
    assert (want["route"][kind == 2] < nh).all()
    zero = want["replies"][int(want["bin_first"][nh + 1]):]
    assert len(zero) == 100 and not zero.tobytes().strip(b"\0")
    served = want["calls_out"][:int(want["bin_first"][nh])]
    assert (served["payload_off"] > 1 << 32).all() and served["cred_ref"].any() and served["verf_ref"].any()


BAD_OWN = [(1, 9, 9, 0, 0, 0), (1, 9, TOP, 2, 0, 1), (1, 9, 0, 1, 0, 2), (1, 9, 0, 5, 0, 0), (1, 9, 0, 1, 4, 1)]
BAD_PAIR = [((5, 5, 5, 1, 0, 0), (5, 5, 5, 1, 0, 0)), ((5, 5, 5, 1, 0, 0), (5, 5, 4, 1, 0, 0)),
            ((5, 5, 5, 1, 0, 0), (5, 4, 9, 1, 0, 0)), ((H31, 5, 5, 1, 0, 0), (H31 - 1, 5, 5, 1, 0, 0)),
            ((5, 5, 5, 3, 0, 0), (5, 5, 7, 1, 0, 0))]


def test_bad_tables(R, codec):
    nh = 4
    m, status = records_for(np.arange(70) % 3 + nh, nh, {}, seed=4)
    seen = set()
    for row in BAD_OWN:
        for at in (0, 2, 4):
            rows = [(10 + i, 0, 0, 1, 0, 0) for i in range(5)]
            rows[at] = (10 + at,) + row[1:]
            want = _check(R, codec, m, status, M.table(rows), nh, f"bad entry {row} at {at}")
            assert want["result"].tolist() == [0, 0, 0, at + 1] and not want["bin_first"].any()
            seen.add(at + 1)
    for a, b in BAD_PAIR:
        for at in (0, 2, 3):
            rows = [(1, 0, 0, 1, 0, 0), (2, 0, 0, 1, 0, 0), (3, 0, 0, 1, 0, 0), (4, 0, 0, 1, 0, 0), (TOP, 0, 0, 1, 0, 0)]
            rows[at], rows[at + 1] = a, b
            if at == 0:
                rows[2:] = [(TOP - 2, 0, 0, 1, 0, 0), (TOP - 1, 0, 0, 1, 0, 0), (TOP, 0, 0, 1, 0, 0)]
            want = _check(R, codec, m, status, M.table(rows), nh, f"bad pair {a} {b} at {at}")
            assert want["result"].tolist() == [0, 0, 0, at + 1] and not want["bin_first"].any()
    assert seen == {1, 3, 5}
    # nh == 0 admits only the empty table; the last entry of 1024; and no records at all
    want = _check(R, codec, m, status, M.table([(1, 1, 1, 1, 0, 1)]), 0, "an entry with nh 0")
    assert want["result"].tolist() == [0, 0, 0, 1]
    rows, _ = make_table(253, 1024)
    rows[1023] = rows[1023][:5] + (3,)
    assert _check(R, codec, m, status, M.table(rows), 253, "entry 1023")["result"].tolist() == [0, 0, 0, 1024]
    assert _check(R, codec, m[:0], status[:0], M.table(rows), 253, "entry 1023, n 0")["result"].tolist() == [0, 0, 0, 1024]


def _reply_batch(replies):
    return L.HostBatch(np.ascontiguousarray(replies), np.zeros(1, L.UNIX_DTYPE), np.zeros(1, np.uint8),
                       np.zeros(1, np.uint8))


def test_encode_of_the_rejected_slice(R, codec, oracle, golden):
    nh = 5
    tab = M.table([(200, 2, 0, 4, 0, 0), (200, 3, 0, 4, 0, 0), (200, 7, 0, 1, 4, 1), (300, 3, 0, 1, 0, 0),
                   (300, 9, 0, 1, 0, 0)])
    keys = [(200, 2, 1), (200, 1, 0), (200, 4, 0), (9, 9, 9), (200, 8, 0), (200, 3, 4), (300, 5, 0), (200, 7, 0),
            (300, 9, 1)]
    m = M.calls(keys, xid0=0x1E - 6)                           # (the golden vectors' xids: 0x1e, then 0x15 below)
    m["xid"][8] = 0x15
    want = _check(R, codec, m, np.zeros(len(m), np.int32), tab, nh, "rejected slice")
    g = R.route_calls_host(codec, m, np.zeros(len(m), np.int32), tab, nh)
    lo, hi = int(g["bin_first"][nh]), int(g["bin_first"][nh + 1])
    assert (lo, hi) == (2, 9)
    wire, off, st, _ = R.encode_host_batch(codec, _reply_batch(g["replies"][lo:hi]))
    o_wire, o_off, o_st, _ = oracle.encode_batch(_reply_batch(want["replies"][lo:hi]))
    assert not st.any() and not o_st.any()
    assert np.array_equal(off, o_off) and wire == o_wire
    stats = [M.PROG_MISMATCH, M.PROG_MISMATCH, M.PROG_UNAVAIL, M.PROG_MISMATCH, M.PROC_UNAVAIL, M.PROG_MISMATCH,
             M.PROC_UNAVAIL]
    lows = [(2, 7), (2, 7), (0, 0), (2, 7), (0, 0), (3, 9), (0, 0)]
    w = np.frombuffer(wire + b"\0" * 16, np.uint8).copy()
    for mode in (L.DECODE_SLICE, L.DECODE_BYTES):
        dm, _, ds, _, _ = R.decode_host_wire(codec, w, off, mode)
        assert not ds.any()
        assert dm["msg_type"].tolist() == [1] * 7 and dm["reply_stat"].tolist() == [0] * 7
        assert dm["stat"].tolist() == stats
        assert list(zip(dm["f0"].tolist(), dm["f1"].tolist())) == lows
        assert dm["xid"].tolist() == m["xid"][want["order"][lo:hi]].tolist()
    # the golden replies of the same shape (an AUTH_NONE verifier): the bytes after the xid, and the whole record
    vec = {v["name"]: bytes.fromhex(v["hex"]) for v in golden["xdrlib"]}
    rec = [wire[int(off[i]):int(off[i + 1])] for i in range(7)]
    assert rec[5] == vec["reply_prog_mismatch"] and rec[6] == vec["reply_proc_unavail"]
    assert rec[4][8:] == vec["reply_proc_unavail"][8:]
    assert rec[2][8:24] == vec["reply_proc_unavail"][8:24] and rec[2][24:] == struct.pack(">I", M.PROG_UNAVAIL)


def test_end_to_end_300_records(R, codec, oracle):
    nh = 7
    rows = [(100003, 3, 0, 4, 0, 0), (100003, 3, 6, 10, 4, 1), (100003, 4, 0, 2, 5, 0), (100005, 3, 0, 6, 6, 1)]
    tab = M.table(rows)
    rng = np.random.default_rng(33)
    msgs = S.random_messages(300, seed=77, max_payload=300)
    progs = [(100003, 3), (100003, 3), (100003, 4), (100005, 3), (100003, 2), (100005, 1), (100021, 4), (391002, 1)]
    for d in msgs:
        if d["type"] == "call" and rng.random() < 0.9:        # (the rest keep their random programs)
            d["program"], d["program_version"] = progs[int(rng.integers(0, len(progs)))]
            d["procedure"] = int(rng.integers(0, 18))
    wire, off, st, _ = R.encode_host_batch(codec, L.build_batch(msgs))
    assert not st.any()
    # four connections' buffers, cut at record boundaries, scattered in a slab with gaps
    cuts = [0, 61, 150, 151, 300]
    slab, seg_off, seg_len = bytearray(), [], []
    for s in (2, 0, 3, 1):
        slab += b"\xEE" * (13 + 7 * s)
        seg_off.append(len(slab))
        part = wire[int(off[cuts[s]]):int(off[cuts[s + 1]])]
        seg_len.append(len(part))
        slab += part
    arrival = [i for s in (2, 0, 3, 1) for i in range(cuts[s], cuts[s + 1])]
    rec_start, rec_len, _, _, res = R.frame_host_streams(codec, bytes(slab), seg_off, seg_len)
    assert int(res[0]) == 300
    w = np.frombuffer(bytes(slab) + b"\0" * 16, np.uint8).copy()
    dm, _, ds, _, _ = R.decode_host_extents(codec, w, rec_start, rec_len, L.DECODE_SLICE, wire_len=len(slab))
    assert not ds.any() and dm["xid"].tolist() == [msgs[i]["xid"] for i in arrival]
    want = _check(R, codec, dm, ds, tab, nh, "end to end")
    g = R.route_calls_host(codec, dm, ds, tab, nh)
    # each handler's slice: exactly that handler's Calls, in arrival order (worked out from the messages themselves)
    mine = {b: [] for b in range(nh + 3)}
    for k, i in enumerate(arrival):
        d = msgs[i]
        b = M.lookup(tab, nh, d["program"], d["program_version"], d["procedure"])[0] if d["type"] == "call" else nh + 1
        mine[b].append(k)
    assert sum(len(mine[h]) for h in range(nh)) > 15 and len(mine[nh]) > 30      # (the input has both kinds)
    for b in range(nh + 3):
        lo, hi = int(g["bin_first"][b]), int(g["bin_first"][b + 1])
        assert g["order"][lo:hi].tolist() == mine[b]
        assert g["calls_out"][lo:hi].tobytes() == dm[np.array(mine[b], np.int64)].tobytes()
    lo, hi = int(g["bin_first"][nh]), int(g["bin_first"][nh + 1])
    r_wire, r_off, r_st, _ = R.encode_host_batch(codec, _reply_batch(g["replies"][lo:hi]))
    o_wire, o_off, o_st, _ = oracle.encode_batch(_reply_batch(want["replies"][lo:hi]))
    assert not r_st.any() and not o_st.any() and np.array_equal(r_off, o_off) and r_wire == o_wire
    # a handler's skeletons: its Calls' xids, Success, nothing else
    sk = g["replies"][:lo]
    assert sk["xid"].tolist() == dm["xid"][g["order"][:lo]].tolist() and (sk["msg_type"] == 1).all()
    assert not sk["stat"].any() and not sk["payload_len"].any()


def test_graph_capture_and_replay(R):
    import torch
    nh, n = 9, 2 * T + 77
    rows, key_of = make_table(nh, 5)
    tab = M.table(rows)
    reach = reachable(nh, key_of)
    d_msgs = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    route = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    order = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    bin_first = torch.full((nh + 5,), -1, dtype=torch.int64, device="cuda")
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    calls = torch.full(((n + 1) * 64,), SENT, dtype=torch.uint8, device="cuda")
    reps = torch.full(((n + 1) * 64,), SENT, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def work(codec):
        codec.route_calls(d_msgs, d_st, n, d_tab, len(tab), nh, route, order, bin_first, res, calls_out=calls,
                          replies=reps)

    fresh = R.Codec(0, stream=s.cuda_stream)
    codec = R.Codec(0, stream=s.cuda_stream)
    try:
        # without the reserve, the call would grow its scratch inside the capture: refused, nothing launched
        err = None
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            try:
                work(fresh)
            except R.CodecError as e:
                err = str(e)
        assert err is not None and "rc=-5" in err, err
        torch.cuda.synchronize()
        assert (route == -1).all().item() and (res == -1).all().item() and (reps == SENT).all().item()
        codec.reserve(n)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            work(codec)                              # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            work(codec)
        torch.cuda.synchronize()
        for seed in (5, 6):
            rng = np.random.default_rng(seed)
            m, st = records_for(reach[rng.integers(0, len(reach), n)], nh, key_of, seed=seed)
            d_msgs.copy_(torch.from_numpy(m.view(np.uint8).reshape(-1).copy()).cuda())
            d_st.copy_(torch.from_numpy(st.copy()).cuda())
            for t in (route, order, bin_first, res):
                t.fill_(-1)
            calls.fill_(SENT)
            reps.fill_(SENT)
            g.replay()
            torch.cuda.synchronize()
            want = M.route_calls(m, st, tab, nh)
            assert res.cpu().numpy().view(np.uint64).tolist() == want["result"].tolist() + [int(U64)]
            assert np.array_equal(bin_first.cpu().numpy().view(np.uint64)[:nh + 4], want["bin_first"])
            assert np.array_equal(route.cpu().numpy().view(np.uint32)[:n], want["route"])
            assert np.array_equal(order.cpu().numpy().view(np.uint32)[:n], want["order"])
            assert calls.cpu().numpy()[:64 * n].tobytes() == want["calls_out"].tobytes()
            assert reps.cpu().numpy()[:64 * n].tobytes() == want["replies"].tobytes()
            assert (calls.cpu().numpy()[64 * n:] == SENT).all() and (reps.cpu().numpy()[64 * n:] == SENT).all()
            assert route[n].item() == -1 and order[n].item() == -1 and bin_first[nh + 4].item() == -1
    finally:
        fresh.close()
        codec.close()


def test_cpp_mirror(R, codec, tmp_path, oracle):
    """RouteTable / route_calls / RoutedCalls::reject_replies of
    include/onc_rpc.hpp (tests/cpp_route/test_route.cpp) over a wire and a
    table written here; its summary is compared with the model's."""
    exe = os.path.join(ROOT, "tests", "cpp_route", "test_route")
    assert os.path.exists(exe), "build() compiles tests/cpp_route"
    nh = 6
    rows = [(100005, 3, 0, 6, 5, 1), (100003, 4, 0, 2, 4, 1), (100003, 3, 6, 10, 3, 1), (100003, 3, 0, 3, 0, 0)]   # unsorted
    tab = M.table(sorted(rows))
    rng = np.random.default_rng(12)
    msgs = S.random_messages(200, seed=5, max_payload=64)
    progs = [(100003, 3), (100003, 4), (100005, 3), (100003, 2), (100005, 9), (391002, 1)]
    for d in msgs:
        if d["type"] == "call":
            d["program"], d["program_version"] = progs[int(rng.integers(0, len(progs)))]
            d["procedure"] = int(rng.integers(0, 18))
    wire, off, st, _ = oracle.encode_batch(L.build_batch(msgs))
    assert not st.any()
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<QQQ", nh, len(rows), len(wire)))
        for row in rows:
            f.write(struct.pack("<6I", *row))
        f.write(wire)
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS test_route" in r.stdout, r.stdout + r.stderr
    w = np.frombuffer(wire + b"\0" * 16, np.uint8).copy()
    dm, _, ds, _, _ = oracle.decode_batch(w, off, L.DECODE_SLICE)
    want = M.route_calls(dm, ds, tab, nh)
    lo, hi = int(want["bin_first"][nh]), int(want["bin_first"][nh + 1])
    o_wire, _, _, _ = oracle.encode_batch(_reply_batch(want["replies"][lo:hi]))
    blob = open(outp, "rb").read()
    n, nbins = struct.unpack_from("<QQ", blob, 0)
    assert (n, nbins) == (200, nh + 3)
    at = 16
    first = np.frombuffer(blob, np.uint64, nh + 4, at)
    at += 8 * (nh + 4)
    order = np.frombuffer(blob, np.uint32, n, at)
    at += 4 * n
    xids = np.frombuffer(blob, np.uint32, n, at)
    at += 4 * n
    (rlen,) = struct.unpack_from("<Q", blob, at)
    assert np.array_equal(first, want["bin_first"]) and np.array_equal(order, want["order"])
    assert np.array_equal(xids, want["calls_out"]["xid"])
    assert blob[at + 8:at + 8 + rlen] == o_wire and len(blob) == at + 8 + rlen
