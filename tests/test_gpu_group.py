"""A send batch grouped by connection on the GPU: onc_group_by_conn and
onc_conn_extents (group.hip) against their host model (tests/group_model.py,
itself checked on the CPU in tests/test_group_model.py). Every output array is
compared whole and bit-exactly, with the optional arguments given and not
given, and every device output is pre-filled with a sentinel with guard words
behind it: a stray write fails by comparison. rec_conn is followed on the
device by words of connection 0, so an item whose index lies outside rec_conn
and is read all the same lands in group 0 instead of the dropped group."""
import os
import struct
import subprocess

import numpy as np
import pytest

import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
import group_model as M
import route_model as RM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
S32, S64 = 0xA5A5A5A5, np.uint64(0xA5A5A5A5A5A5A5A5)
TOP = 0xFFFFFFFF
T = 1024


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


def descriptors(n, seed=0):
    """n descriptors of random bytes whose payload_off lies above 2^32."""
    rng = np.random.default_rng(1000 + seed)
    m = np.frombuffer(rng.integers(0, 256, 64 * n, dtype=np.uint8).tobytes(), L.MSG_DTYPE).copy()
    m["payload_off"] = (np.arange(n, dtype=np.uint64) << np.uint64(33)) | np.uint64(0x100000001)
    return m


def _check(R, codec, rec_conn, via, nconn, what, with_msgs=(False, True)):
    """onc_group_by_conn with and without the descriptors against the model -> the model's result."""
    rec_conn = np.asarray(rec_conn, np.uint32)
    n = len(rec_conn) if via is None else len(via)
    msgs = descriptors(n, seed=n)
    want = M.group(rec_conn, via, nconn, msgs=msgs)
    for on in with_msgs:
        g = R.group_by_conn_host(codec, rec_conn, via, nconn, msgs=msgs if on else None)
        raw, w = g["raw"], f"{what} (n {n}, nconn {nconn}, via {via is not None}, msgs_out {on})"
        assert g["result"].tolist() == want["result"].tolist(), f"{w}: result {g['result']} != {want['result']}"
        assert (raw["result"][3:] == S64).all(), f"{w}: result written past 3"
        assert np.array_equal(g["conn_first"], want["conn_first"]), f"{w}: conn_first"
        assert (raw["conn_first"][nconn + 2:] == S64).all(), f"{w}: conn_first written past nconn + 2"
        assert np.array_equal(g["order"], want["order"]), f"{w}: order"
        assert (raw["order"][n:] == S32).all(), f"{w}: order written past n"
        if on:
            assert g["msgs_out"].tobytes() == want["msgs_out"].tobytes(), f"{w}: msgs_out"
            assert (raw["msgs_out"][64 * n:] == SENT).all(), f"{w}: msgs_out written past n"
        else:
            assert g["msgs_out"] is None
        if n:
            # stability, directly: order is strictly increasing inside each group, and a permutation
            o, first = g["order"].astype(np.int64), g["conn_first"].astype(np.int64)
            inside = np.ones(n, bool)
            inside[first[(first > 0) & (first < n)]] = False
            assert (np.diff(o)[inside[1:]] > 0).all(), f"{w}: order not ascending inside a group"
            assert np.array_equal(np.sort(o), np.arange(n)), f"{w}: order is no permutation"
    return want


def conns_for(n, nconn, seed):
    """Connections over the whole range, a few of them busy, some items dropped."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, nconn + 1, n).astype(np.uint32)                 # (nconn itself: dropped)
    busy = rng.integers(0, nconn + 1, 5).astype(np.uint32)
    pick = rng.random(n) < 0.4
    c[pick] = busy[rng.integers(0, 5, n)][pick]
    c[rng.random(n) < 0.05] = TOP
    return c


SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1)
NCONNS = (0, 1, 2, 255, 256, 257, 65535, 65536, 65537)


def test_tile_constant(R):
    assert R.GROUP_TILE == T == M.TILE and R.GROUP_CONN_MAX == M.CONN_MAX


def test_no_items_on_a_fresh_handle(R):
    c = R.Codec(0)
    try:
        for nconn in (3, 0):
            g = R.group_by_conn_host(c, [], None, nconn)
            assert g["conn_first"].tolist() == [0] * (nconn + 2) and g["result"].tolist() == [0, 0, 0]
            assert (g["raw"]["order"] == S32).all() and (g["raw"]["conn_first"][nconn + 2:] == S64).all()
    finally:
        c.close()


@pytest.mark.parametrize("nconn", NCONNS)
def test_sizes(R, codec, nconn):
    assert M.passes(nconn) == {0: 0, 1: 1, 2: 1, 255: 1, 256: 2, 257: 2, 65535: 2, 65536: 3, 65537: 3}[nconn]
    for n in SIZES:
        rc = conns_for(n, nconn, seed=n + nconn)
        _check(R, codec, rc, None, nconn, "sizes")
        # through via: a permutation of a longer rec_conn
        src = conns_for(n + 9, nconn, seed=n + nconn + 1)
        via = np.random.default_rng(n).permutation(n + 9)[:n].astype(np.uint32)
        _check(R, codec, src, via, nconn, "sizes, via")


def test_the_most_connections(R, codec):
    nconn = (1 << 24) - 1
    rc = conns_for(100, nconn, seed=3)
    rc[:4] = [nconn - 1, nconn, 0, nconn - 1]
    want = _check(R, codec, rc, None, nconn, "2^24 - 1 connections")
    assert int(want["result"][2]) > 30


def test_distributions(R, codec):
    n, nconn = 3 * T + 1, 70000
    assert M.passes(nconn) == 3
    k = np.arange(n, dtype=np.uint32)
    cases = {
        "one connection": np.full(n, 4242, np.uint32),
        "all dropped": np.full(n, TOP, np.uint32),
        "descending": (nconn - 1 - k).astype(np.uint32),
        "top digit alternates": np.where(k & 1, 0x10001, 0x00001).astype(np.uint32),
        "middle digit alternates": np.where(k & 1, 0x00101, 0x00001).astype(np.uint32),
        "low digit alternates": np.where(k & 1, 0x00002, 0x00001).astype(np.uint32),
        "equal low two digits": ((k % 2).astype(np.uint32) << 16) | 0x0034,
        "300 connections in turn": (k % 300).astype(np.uint32) * 233,
        "the highest first": np.concatenate([[nconn - 1], np.zeros(n - 1)]).astype(np.uint32),
        "dropped ids mixed in": np.array([nconn, nconn + 1, TOP, 5, nconn - 1, 65536], np.uint32)[k % 6],
    }
    for what, rc in cases.items():
        assert len(rc) == n and rc.dtype == np.uint32
        want = _check(R, codec, rc, None, nconn, what)
        assert int(want["conn_first"][nconn + 1]) == n
    assert M.group(cases["all dropped"], None, nconn)["result"].tolist() == [0, n, 0]
    assert M.group(cases["300 connections in turn"], None, nconn)["result"].tolist() == [n, 0, 300]
    assert M.group(cases["dropped ids mixed in"], None, nconn)["result"].tolist()[2] == 3


def test_via(R, codec):
    rng = np.random.default_rng(21)
    for nconn in (7, 300, 70000):
        nsrc = 2 * T + 5
        src = conns_for(nsrc, nconn, seed=nconn)
        _check(R, codec, src, rng.permutation(nsrc).astype(np.uint32), nconn, "via: a permutation")
        _check(R, codec, src, rng.integers(0, 40, T + 3).astype(np.uint32), nconn, "via: repeats")
        # entries at nsrc, nsrc + 1 and 0xFFFFFFFF are dropped and rec_conn is not read there: the words behind it
        # on the device say connection 0
        via = rng.integers(0, nsrc, T + 70).astype(np.uint32)
        via[[0, 63, 64, T - 1, T, T + 69]] = [nsrc, nsrc + 1, TOP, nsrc, TOP, nsrc + 1]
        via[100:140] = nsrc
        want = _check(R, codec, src, via, nconn, "via: outside rec_conn")
        assert int(want["result"][1]) >= 46
        # nothing to read at all
        want = _check(R, codec, np.zeros(0, np.uint32), np.array([0, 1, TOP, 5], np.uint32), nconn, "via: nsrc 0")
        assert want["result"].tolist() == [0, 4, 0] and want["order"].tolist() == [0, 1, 2, 3]


def test_descriptor_gather(R, codec):
    n, nconn = 2 * T + 3, 500
    rc = conns_for(n, nconn, seed=8)
    msgs = descriptors(n, seed=4)
    assert (msgs["payload_off"] > 1 << 32).all()
    g = R.group_by_conn_host(codec, rc, None, nconn, msgs=msgs, extra=8)
    assert g["msgs_out"].tobytes() == msgs[g["order"]].tobytes()
    assert (g["raw"]["msgs_out"][64 * n:] == SENT).all() and len(g["raw"]["msgs_out"]) == 64 * (n + 8)
    # msgs is indexed by item, not through via
    via = np.random.default_rng(2).integers(0, n, T + 1).astype(np.uint32)
    g = R.group_by_conn_host(codec, rc, via, nconn, msgs=msgs[:T + 1])
    want = M.group(rc, via, nconn, msgs=msgs[:T + 1])
    assert np.array_equal(g["order"], want["order"]) and g["msgs_out"].tobytes() == want["msgs_out"].tobytes()


def _reply_batch(replies, arena):
    return L.HostBatch(np.ascontiguousarray(replies), np.zeros(1, L.UNIX_DTYPE), np.zeros(1, np.uint8), arena)


def test_conn_extents(R, codec):
    # the rec_off of a real encode; connections 0, 1 (the start), 5, 6 (the middle) and 10, 11 (the end) are empty
    nconn = 12
    rng = np.random.default_rng(17)
    msgs = S.random_messages(200, seed=9, max_payload=120)
    hb = L.build_batch(msgs)
    wire, off, st, _ = R.encode_host_batch(codec, hb)
    assert not st.any()
    rc = rng.choice(np.array([2, 3, 4, 7, 8, 9, nconn, TOP], np.uint32), 200)
    g = R.group_by_conn_host(codec, rc, None, nconn, msgs=hb.msgs)
    want = M.group(rc, None, nconn)
    assert np.array_equal(g["conn_first"], want["conn_first"])
    sent = int(g["result"][0])
    assert 0 < sent < 200 and int(g["result"][2]) == 6
    # the grouped batch, encoded whole and only its sent part
    grouped = L.HostBatch(g["msgs_out"], hb.unix, hb.auth_arena, hb.payload_arena)
    g_wire, g_off, g_st, _ = R.encode_host_batch(codec, grouped)
    assert not g_st.any() and len(g_wire) == len(wire)
    for nrec in (200, sent, sent - 1, 0):
        ro = g_off[:nrec + 1]
        got, raw = R.conn_extents_host(codec, ro, g["conn_first"], nconn, nrec=nrec)
        assert np.array_equal(got, M.conn_extents(ro, nrec, want["conn_first"])), nrec
        assert (raw[nconn + 2:] == S64).all()
        if nrec >= sent:
            # every connection's bytes are its records, in the order they were given
            for c in range(nconn):
                mine = b"".join(wire[int(off[k]):int(off[k + 1])] for k in np.flatnonzero(rc == c))
                assert g_wire[int(got[c]):int(got[c + 1])] == mine, (nrec, c)
            assert int(got[0]) == 0 and int(got[nconn]) == int(g_off[sent])
            assert int(got[nconn + 1]) == int(g_off[nrec])
    for c in (0, 1, 5, 6, 10, 11):
        assert int(want["conn_first"][c]) == int(want["conn_first"][c + 1])


def test_mapped_host_memory(R, codec):
    import torch
    n, nsrc, nconn = T + 37, T + 50, 300
    rng = np.random.default_rng(31)
    src = conns_for(nsrc, nconn, seed=6)
    via = rng.integers(0, nsrc + 2, n).astype(np.uint32)
    msgs = descriptors(n, seed=7)
    want = M.group(src, via, nconn, msgs=msgs)
    h_src = R.HostMapped.from_array(codec, src)
    h_via = R.HostMapped.from_array(codec, via)
    h_order = R.HostMapped(codec, 4 * (n + 4))
    h_first = R.HostMapped(codec, 8 * (nconn + 2 + 4))
    h_out = R.HostMapped(codec, 64 * (n + 4))
    try:
        for h in (h_order, h_first, h_out):
            h.host[:] = SENT
        d_msgs = R.to_device(msgs, "cuda")
        res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        codec.group_by_conn(h_src, nsrc, h_via, n, nconn, h_order, h_first, res, msgs=d_msgs, msgs_out=h_out)
        codec.sync()
        assert res.cpu().numpy().view(np.uint64)[:3].tolist() == want["result"].tolist() and res[3].item() == -1
        order, first = h_order.host.view(np.uint32), h_first.host.view(np.uint64)
        assert np.array_equal(order[:n], want["order"]) and (order[n:] == S32).all()
        assert np.array_equal(first[:nconn + 2], want["conn_first"]) and (first[nconn + 2:] == S64).all()
        assert h_out.host[:64 * n].tobytes() == want["msgs_out"].tobytes() and (h_out.host[64 * n:] == SENT).all()
    finally:
        for h in (h_src, h_via, h_order, h_first, h_out):
            h.close()


def test_end_to_end_300_records(R, codec, oracle):
    """Four connections' buffers through onc_frame_streams, onc_decode_extents
    and onc_route_calls; the replies grouped with via = order and rec_conn =
    rec_seg, encoded, and cut by onc_conn_extents. The items are in handler
    order and the sort is stable in the items, so a connection's replies come
    handler by handler, the rejected Calls last, and in arrival order inside a
    handler: that is the order the expected bytes are built in, from the
    messages themselves."""
    nh = 7
    rows = [(100003, 3, 0, 4, 0, 0), (100003, 3, 6, 10, 4, 1), (100003, 4, 0, 2, 5, 0), (100005, 3, 0, 6, 6, 1)]
    tab = RM.table(rows)
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
    cuts, slots = [0, 61, 150, 151, 300], (2, 0, 3, 1)
    slab, seg_off, seg_len = bytearray(), [], []
    for s in slots:
        slab += b"\xEE" * (13 + 7 * s)
        seg_off.append(len(slab))
        part = wire[int(off[cuts[s]]):int(off[cuts[s + 1]])]
        seg_len.append(len(part))
        slab += part
    arrival = [i for s in slots for i in range(cuts[s], cuts[s + 1])]
    conn_of = [c for c, s in enumerate(slots) for _ in range(cuts[s], cuts[s + 1])]
    rec_start, rec_len, rec_seg, _, res = R.frame_host_streams(codec, bytes(slab), seg_off, seg_len)
    assert int(res[0]) == 300 and rec_seg.tolist() == conn_of
    w = np.frombuffer(bytes(slab) + b"\0" * 16, np.uint8).copy()
    dm, _, ds, _, _ = R.decode_host_extents(codec, w, rec_start, rec_len, L.DECODE_SLICE, wire_len=len(slab))
    assert not ds.any()
    g = R.route_calls_host(codec, dm, ds, tab, nh)
    ncalls, served = int(g["bin_first"][nh + 1]), int(g["bin_first"][nh])
    # the handlers fill their slices: a result per served Call out of a small arena
    arena = np.random.default_rng(5).integers(0, 256, 256, dtype=np.uint8)
    replies = g["replies"].copy()
    for k in range(served):
        r = int(g["order"][k])
        replies["payload_off"][k], replies["payload_len"][k] = (13 * r) % 200, (7 * r) % 50
    # the replies of the Calls, served and rejected, by connection
    grouped = R.group_by_conn_host(codec, rec_seg, g["order"][:ncalls], 4, msgs=replies[:ncalls])
    sent = int(grouped["result"][0])
    assert sent == ncalls and int(grouped["result"][1]) == 0
    assert np.array_equal(grouped["order"], M.group(rec_seg, g["order"][:ncalls], 4)["order"])
    out = grouped["msgs_out"][:sent]
    r_wire, r_off, r_st, _ = R.encode_host_batch(codec, _reply_batch(out, arena))
    assert not r_st.any()
    conn_off, _ = R.conn_extents_host(codec, r_off, grouped["conn_first"], 4)
    # what each connection must get, from the messages themselves: the reply to each of its Calls, in the items'
    # order, which with via = onc_route_calls' order is handler by handler (the rejected Calls last) and, inside a
    # handler, the order the Calls arrived on the connection
    want_of = {c: [] for c in range(4)}
    for r, i in enumerate(arrival):
        d = msgs[i]
        if d["type"] != "call":
            continue
        b, stat, low, high = RM.lookup(tab, nh, d["program"], d["program_version"], d["procedure"])
        rep = np.zeros(1, L.MSG_DTYPE)
        rep["xid"], rep["msg_type"], rep["stat"] = d["xid"], 1, stat
        if stat == RM.PROG_MISMATCH:
            rep["f0"], rep["f1"] = low, high
        if b < nh:
            rep["payload_off"], rep["payload_len"] = (13 * r) % 200, (7 * r) % 50
        want_of[conn_of[r]].append((b, rep))
    assert sum(len(v) for v in want_of.values()) == ncalls
    assert int(grouped["result"][2]) == sum(1 for v in want_of.values() if v) >= 3
    at = 0
    for c in range(4):
        o_wire = b""                                                    # (a connection that sent no Call)
        if want_of[c]:
            mine = [rep for _, rep in sorted(want_of[c], key=lambda e: e[0])]          # (stable: arrival order inside)
            o_wire, _, o_st, _ = oracle.encode_batch(_reply_batch(np.concatenate(mine), arena))
            assert not o_st.any()
        lo, hi = int(conn_off[c]), int(conn_off[c + 1])
        assert lo == at and r_wire[lo:hi] == o_wire, c                  # the ranges tile the stream
        at = hi
    assert at == len(r_wire) == int(conn_off[4]) == int(conn_off[5])


def test_graph_capture_and_replay(R):
    import torch
    n, nconn = 2 * T + 77, 300
    d_conn = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_msgs = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    order = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    first = torch.full((nconn + 3,), -1, dtype=torch.int64, device="cuda")
    res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    out = torch.full(((n + 1) * 64,), SENT, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def work(codec):
        codec.group_by_conn(d_conn, n, None, n, nconn, order, first, res, msgs=d_msgs, msgs_out=out)

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
        assert (order == -1).all().item() and (first == -1).all().item() and (res == -1).all().item()
        assert (out == SENT).all().item()
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
            rc = conns_for(n, nconn, seed=seed)
            m = descriptors(n, seed=seed)
            d_conn.copy_(torch.from_numpy(rc.view(np.int32).copy()).cuda())
            d_msgs.copy_(torch.from_numpy(m.view(np.uint8).reshape(-1).copy()).cuda())
            for t in (order, first, res):
                t.fill_(-1)
            out.fill_(SENT)
            g.replay()
            torch.cuda.synchronize()
            want = M.group(rc, None, nconn, msgs=m)
            assert res.cpu().numpy().view(np.uint64).tolist() == want["result"].tolist() + [int(np.uint64(2**64 - 1))]
            assert np.array_equal(first.cpu().numpy().view(np.uint64)[:nconn + 2], want["conn_first"])
            assert np.array_equal(order.cpu().numpy().view(np.uint32)[:n], want["order"])
            assert out.cpu().numpy()[:64 * n].tobytes() == want["msgs_out"].tobytes()
            assert (out.cpu().numpy()[64 * n:] == SENT).all()
            assert order[n].item() == -1 and first[nconn + 2].item() == -1
    finally:
        fresh.close()
        codec.close()


def test_cpp_mirror(R, codec, tmp_path, oracle):
    """group_by_conn / GroupedSends::connection_streams of include/onc_rpc.hpp
    (tests/cpp_group/test_group.cpp) over a wire and a connection list written
    here; its summary is compared with the model's."""
    exe = os.path.join(ROOT, "tests", "cpp_group", "test_group")
    assert os.path.exists(exe), "build() compiles tests/cpp_group"
    nconn, n, nsrc = 9, 60, 70
    rng = np.random.default_rng(12)
    msgs = S.random_messages(n, seed=5, max_payload=64)
    wire, off, st, _ = oracle.encode_batch(L.build_batch(msgs))
    assert not st.any()
    conn_of = rng.choice(np.array([0, 2, 3, 3, 7, 8, nconn, TOP], np.uint32), nsrc)
    via = rng.integers(0, nsrc, n).astype(np.uint32)
    via[[5, 40]] = [nsrc, TOP]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<QQQQ", nconn, nsrc, n, len(wire)))
        f.write(conn_of.tobytes() + via.tobytes() + wire)
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS test_group" in r.stdout, r.stdout + r.stderr
    want = M.group(conn_of, via, nconn)
    sent = int(want["result"][0])
    recs = [wire[int(off[k]):int(off[k + 1])] for k in range(n)]
    stream = b"".join(recs[int(k)] for k in want["order"][:sent])
    g_off = np.concatenate([[0], np.cumsum([len(recs[int(k)]) for k in want["order"][:sent]])]).astype(np.uint64)
    ext = M.conn_extents(g_off, sent, want["conn_first"])
    blob = open(outp, "rb").read()
    head = struct.unpack_from("<QQQQ", blob, 0)
    assert list(head) == [n] + want["result"].tolist()
    at = 32
    first = np.frombuffer(blob, np.uint64, nconn + 2, at)
    at += 8 * (nconn + 2)
    order = np.frombuffer(blob, np.uint32, n, at)
    at += 4 * n
    xids = np.frombuffer(blob, np.uint32, n, at)
    at += 4 * n
    ranges = np.frombuffer(blob, np.uint64, 2 * (nconn + 1), at).reshape(-1, 2)
    at += 16 * (nconn + 1)
    (slen,) = struct.unpack_from("<Q", blob, at)
    assert np.array_equal(first, want["conn_first"]) and np.array_equal(order, want["order"])
    assert xids.tolist() == [msgs[int(k)]["xid"] for k in want["order"]]
    assert np.array_equal(ranges[:, 0], ext[:nconn + 1]) and np.array_equal(ranges[:, 1], ext[1:nconn + 2])
    assert blob[at + 8:at + 8 + slen] == stream and len(blob) == at + 8 + slen
