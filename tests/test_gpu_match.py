"""Decoded Replies paired with pending Calls on the GPU: onc_match_replies
(match.hip) against its host model (tests/match_model.py, itself pinned on
the CPU in tests/test_match_model.py). Every output array is compared whole
and bit-exactly, with tag_out and still given and not given, and every device
output is pre-filled with a sentinel with guard elements behind it: a stray
write fails by comparison. Every input is one the interface defines a result
for."""
import os
import struct
import subprocess

import numpy as np
import pytest

import match_model as M
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
S32, S64 = 0xA5A5A5A5, np.uint64(0xA5A5A5A5A5A5A5A5)
H31, TOP = 0x80000000, 0xFFFFFFFF
T = 1024
SIZES = (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1)
ALL4 = ((True, True), (False, False), (True, False), (False, True))


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
def chain(R):
    """A codec whose every key hashes to slot S - 2: one chain that wraps."""
    c = R.Codec(0, variant=R.VARIANT_MATCH_ONE_CHAIN)
    yield c
    c.close()


def _compare(g, want, n, npend, tag_out, still, w):
    raw = g["raw"]
    assert g["result"].tolist() == want["result"].tolist(), f"{w}: result {g['result']} != {want['result']}"
    assert (raw["result"][6:] == S64).all(), f"{w}: result written past 6"
    assert np.array_equal(g["match"], want["match"]), f"{w}: match"
    assert (raw["match"][n:] == S32).all(), f"{w}: match written past n"
    assert np.array_equal(g["hit"], want["hit"]), f"{w}: hit"
    assert (raw["hit"][npend:] == S32).all(), f"{w}: hit written past np"
    if tag_out:
        assert np.array_equal(g["tag_out"], want["tag_out"]), f"{w}: tag_out"
        assert (raw["tag_out"][n:] == S64).all(), f"{w}: tag_out written past n"
    else:
        assert g["tag_out"] is None
    if still:
        k = len(want["still"])
        assert g["still"].tobytes() == want["still"].tobytes(), f"{w}: still"
        assert (raw["still"][k:].view(np.uint8) == SENT).all(), f"{w}: still written past k"
    else:
        assert g["still"] is None


def _check(R, codec, msgs, status, rec_conn, pend, what, combos=ALL4, want=None):
    """onc_match_replies with and without the optional outputs against the model -> the model's result."""
    want = M.match(msgs, status, rec_conn, pend) if want is None else want
    for tag_out, still in combos:
        g = R.match_replies_host(codec, msgs, status, rec_conn, pend, tag_out=tag_out, still=still)
        _compare(g, want, len(msgs), len(pend), tag_out, still, f"{what} (tag_out {tag_out}, still {still})")
    return want


def replies(keys, seed=0):
    """OK Reply descriptors for (conn, xid) keys, every word the call does not
    look at random -> (msgs, status, rec_conn)."""
    rng = np.random.default_rng(seed)
    n = len(keys)
    m = np.frombuffer(rng.bytes(64 * n), L.MSG_DTYPE).copy()
    k = np.asarray(keys, np.uint64).reshape(n, 2)
    m["xid"] = k[:, 1].astype(np.uint32)
    m["msg_type"] = L.MSG_REPLY
    return m, np.zeros(n, np.int32), k[:, 0].astype(np.uint32)


def pending(keys, seed=0):
    """A pending list for (conn, xid) keys with random tags."""
    rng = np.random.default_rng(seed + 1000)
    p = np.zeros(len(keys), L.PENDING_DTYPE)
    k = np.asarray(keys, np.uint64).reshape(len(keys), 2)
    p["conn"], p["xid"] = k[:, 0].astype(np.uint32), k[:, 1].astype(np.uint32)
    p["tag"] = rng.integers(0, 1 << 64, len(keys), dtype=np.uint64)
    return p


def distinct_keys(count, seed=0):
    """`count` different keys: xids counting up from a random start on a handful of connections."""
    rng = np.random.default_rng(seed + 2000)
    conn = rng.integers(0, 1 << 32, 5, dtype=np.uint64)
    x0 = int(rng.integers(0, 1 << 32))
    i = np.arange(count, dtype=np.uint64)
    return np.stack([conn[i % 5], (np.uint64(x0) + i // 5) & np.uint64(TOP)], axis=1)


def test_tile_constant(R):
    assert R.MATCH_TILE == T == M.TILE


def _mixed_case(n, npend, seed, null_conn):
    """A list with repeats and a batch with every outcome, keys from a space small enough that all of them occur."""
    rng = np.random.default_rng(seed)
    space = max(4, (npend * 3) // 4)
    nconn = 1 if null_conn else 3
    pk = np.stack([rng.integers(0, nconn, npend), rng.integers(0, space, npend)], axis=1)
    rk = np.stack([rng.integers(0, nconn, n), rng.integers(0, space + space // 2 + 1, n)], axis=1)
    m, status, rc = replies(rk, seed)
    kind = rng.integers(0, 10, n)
    status[kind == 0] = (1, 10, 106, -3)[seed % 4]
    m["msg_type"][kind == 1] = (L.MSG_CALL, 7)[seed % 2]
    return m, status, (None if null_conn else rc), pending(pk, seed)


def _sizes(R, make_codec, n, nps):
    c = make_codec()
    try:
        for npend in nps:
            for null_conn in (False, True):
                m, status, rc, pend = _mixed_case(n, npend, 31 * n + npend, null_conn)
                want = _check(R, c, m, status, rc, pend, f"n {n} np {npend} rec_conn {'NULL' if null_conn else 'given'}")
                if n >= T - 1 and npend >= 63:
                    assert (want["result"][:5] > 0).all(), "the case has every outcome"
    finally:
        c.close()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(R, n):
    """Every n against every np, each n on a fresh handle without a reserve."""
    _sizes(R, lambda: R.Codec(0), n, SIZES)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_one_chain(R, n):
    _sizes(R, lambda: R.Codec(0, variant=R.VARIANT_MATCH_ONE_CHAIN), n, SIZES[:-1] + (2 * T + 1,))


def test_outcome_mixes(R, codec):
    n = 3 * T + 1
    keys = distinct_keys(n, 1)
    pend = pending(keys, 1)
    rng = np.random.default_rng(2)
    r = np.arange(n)
    other = distinct_keys(n, 99)                     # (another start: not pending)
    assert not set(map(tuple, other.tolist())) & set(map(tuple, keys.tolist()))
    for name, order in (("in list order", r), ("in reverse order", r[::-1]), ("shuffled", rng.permutation(n))):
        m, status, rc = replies(keys[order], 3)
        want = _check(R, codec, m, status, rc, pend, f"all matched {name}")
        assert want["result"].tolist() == [n, 0, 0, 0, 0, 0] and np.array_equal(want["match"], order)
    m, status, rc = replies(other, 4)
    assert _check(R, codec, m, status, rc, pend, "all unknown")["result"].tolist() == [0, n, 0, 0, 0, n]

    def batch(cls, seed):
        """Record r of class cls[r]: 0 matched (entry r), 1 unknown, 2 duplicate (of record 0's entry), 3 not a Reply,
        4 failed. Record 0 is matched wherever a duplicate follows."""
        k = np.where((cls == 1)[:, None], other, keys)
        k[cls == 2] = keys[0]
        m, status, rc = replies(k, seed)
        m["msg_type"][cls == 3] = np.where(r[cls == 3] % 2 == 0, L.MSG_CALL, 7)
        status[cls == 4] = 106
        return m, status, rc

    for c in range(5):
        only = np.full(n, c)
        if c == 2:
            only[0] = 0
        want = _check(R, codec, *batch(only, 10 + c), pend, f"class {c} only", combos=ALL4[:2])
        assert int(want["result"][c]) == n - (c == 2)
        for rest in range(5):                        # class c holding all but one record, the one in the middle
            if rest == c or (rest == 2 and c != 0) or (c == 2 and rest != 0):
                continue
            cls = np.full(n, c)
            cls[0 if c == 2 else T + 5] = rest
            if rest == 2:
                cls[T + 5] = 2
            want = _check(R, codec, *batch(cls, 20 + c), pend, f"class {c} but one of {rest}", combos=ALL4[:1])
            assert int(want["result"][c]) == n - 1 and int(want["result"][rest]) == 1
    cls = r % 5
    cls[0] = 0
    want = _check(R, codec, *batch(cls, 30), pend, "classes alternating")
    assert (want["result"][:5] >= n // 5 - 1).all()


def _repeats_in_list(R, codec, what):
    for k in (2, 64, 65, T + 1):
        # the key k times from entry 3 on with others in between at the wave and tile edges, one Reply
        keys = distinct_keys(k + 40, k)
        at = np.concatenate([[3], 4 + np.sort(np.random.default_rng(k).choice(k + 35, k - 1, replace=False))])
        keys[at] = (7, 77)
        pend = pending(keys, k)
        m, status, rc = replies([(9, 9), (7, 77), (7, 78)], k)
        want = _check(R, codec, m, status, rc, pend, f"{what}: a key {k} times")
        assert want["match"].tolist() == [M.UNKNOWN, 3, M.UNKNOWN] and int(want["hit"][3]) == 1
        assert (want["hit"] != M.NONE).sum() == 1 and len(want["still"]) == k + 39
        assert want["still"]["tag"].tolist() == np.delete(pend["tag"], 3).tolist()
        # every entry the same key
        same = pending([(TOP, 5)] * k, k + 1)
        m, status, rc = replies([(TOP, 5)], k)
        want = _check(R, codec, m, status, rc, same, f"{what}: {k} entries of one key")
        assert want["match"].tolist() == [0] and want["still"].tobytes() == same[1:].tobytes()


def test_repeats_in_list(R, codec):
    _repeats_in_list(R, codec, "plain")


def test_repeats_in_list_one_chain(R, chain):
    _repeats_in_list(R, chain, "one chain")


def _repeats_in_batch(R, codec, what):
    keys = distinct_keys(70, 8)
    pend = pending(keys, 8)
    for k in (64, 65, T + 1):
        # k Replies to entry 5, the first of them record 2, others in between
        rk = distinct_keys(k + 30, 8)[::-1].copy()   # (entries 0 .. 69 where the list has them, the rest unknown)
        dup = 2 + np.sort(np.random.default_rng(k).choice(k + 27, k - 1, replace=False)) + 1
        rk[np.concatenate([[2], dup])] = keys[5]
        m, status, rc = replies(rk, k)
        want = _check(R, codec, m, status, rc, pend, f"{what}: {k} Replies to one Call")
        assert int(want["hit"][5]) == 2 and int(want["match"][2]) == 5
        assert (want["match"] == M.DUPLICATE).sum() >= k - 2 and (want["match"][dup] == M.DUPLICATE).all()
    # the winner the last record of a tile, and the first record of the next
    for win in (T - 1, T):
        rk = np.tile(keys[:1] ^ 1, (2 * T + 3, 1))   # (not pending)
        rk[win:] = keys[9]
        m, status, rc = replies(rk, win)
        want = _check(R, codec, m, status, rc, pend, f"{what}: the winner record {win}", combos=ALL4[:2])
        assert int(want["hit"][9]) == win and (want["match"][win + 1:] == M.DUPLICATE).all()
        assert (want["match"][:win] == M.UNKNOWN).all()


def test_repeats_in_batch(R, codec):
    _repeats_in_batch(R, codec, "plain")


def test_repeats_in_batch_one_chain(R, chain):
    _repeats_in_batch(R, chain, "one chain")


def test_keys(R, codec, chain):
    edge = (0, 0x7FFFFFFF, H31, TOP)
    keys = [(c, x) for c in edge for x in edge]                     # every pair, the swapped ones among them
    keys += [(c, 500) for c in range(70)] + [(500, x) for x in range(70)]     # differing in one word only
    keys += [(1, 2), (2, 1), (3, 1), (1, 3)]
    assert len(set(keys)) == len(keys)
    pend = pending(keys, 3)
    miss = [(1, 0), (0, 1), (TOP, TOP - 1), (TOP - 1, TOP), (H31, 1), (501, 500), (500, 501), (70, 500), (500, 70),
            (2, 2), (0x7FFFFFFE, H31)]
    order = np.random.default_rng(4).permutation(len(keys))
    rk = [keys[i] for i in order] + miss
    for c, name in ((codec, "plain"), (chain, "one chain")):
        m, status, rc = replies(rk, 5)
        want = _check(R, c, m, status, rc, pend, f"keys, {name}")
        assert want["match"][:len(keys)].tolist() == order.tolist() and (want["match"][len(keys):] == M.UNKNOWN).all()
        # rec_conn NULL: only the entries on connection 0 can be hit
        want = _check(R, c, m, status, None, pend, f"keys without rec_conn, {name}")
        hit = np.flatnonzero(want["hit"] != M.NONE)
        assert len(hit) and (pend["conn"][hit] == 0).all()


def test_not_looked_at(R, codec):
    n = 400
    keys = distinct_keys(n, 6)
    pend = pending(keys, 6)
    pend["tag"][:4] = (0, 2**64 - 1, 1, 2**63)
    rng = np.random.default_rng(7)
    m, status, rc = replies(keys, 7)                  # random reply_stat / stat / payload / auth words on every Reply
    kind = np.arange(n) % 4
    # 1: failed records with random descriptor bytes and rec_conn, among them ones that would match
    bad = kind == 1
    m[bad] = np.frombuffer(rng.bytes(64 * int(bad.sum())), L.MSG_DTYPE)
    status[bad] = np.array([(1, 2, 10, 106, -1)[i % 5] for i in range(int(bad.sum()))], np.int32)
    rc[bad] = rng.integers(0, 1 << 32, int(bad.sum()))
    keep = np.flatnonzero(bad)[::3]                   # ... whose key is a pending one, as a Reply
    m["xid"][keep], m["msg_type"][keep], rc[keep] = keys[keep, 1], L.MSG_REPLY, keys[keep, 0]
    # 2: denied Replies answer their Calls as well
    m["reply_stat"][kind == 2], m["stat"][kind == 2] = L.REPLY_DENIED, 1
    want = _check(R, codec, m, status, rc, pend, "not looked at")
    assert (want["match"][bad] == M.FAILED).all() and np.array_equal(want["match"][~bad], np.arange(n)[~bad])
    assert want["tag_out"][:4].tolist() == [0, 0, 1, 2**63] and int(want["tag_out"][4]) == int(pend["tag"][4])
    assert len(want["still"]) == int(bad.sum())
    # the tags 0 and 2^64 - 1 through tag_out: entries 0 and 1 answered
    m, status, rc = replies(keys[:2][::-1], 8)
    want = _check(R, codec, m, status, rc, pend, "tags")
    assert want["tag_out"].tolist() == [2**64 - 1, 0]


def test_successive_batches(R, codec):
    rng = np.random.default_rng(21)
    keys = distinct_keys(5000, 21)
    pend, sent = pending(keys[:1500], 21), 1500
    for rnd in range(3):
        # Replies to about half of what is pending, shuffled, a few twice, a few unknown
        pick = rng.permutation(len(pend))[:len(pend) // 2]
        rk = np.stack([pend["conn"][pick], pend["xid"][pick]], axis=1).astype(np.uint64)
        rk = np.concatenate([rk, rk[:20], keys[4900 + 10 * rnd:4910 + 10 * rnd]])
        m, status, rc = replies(rk[rng.permutation(len(rk))], rnd)
        want = _check(R, codec, m, status, rc, pend, f"round {rnd}")
        g = R.match_replies_host(codec, m, status, rc, pend)
        assert int(want["result"][0]) > 500 and int(want["result"][2]) >= 1 and int(want["result"][1]) == 10
        # the next list: what the device left waiting, then new Calls, some reusing an xid that is still pending
        fresh = keys[sent:sent + 700].copy()
        fresh[::7] = np.stack([g["still"]["conn"][:100], g["still"]["xid"][:100]], axis=1)
        sent += 700
        pend = np.concatenate([g["still"], pending(fresh, 50 + rnd)])
        assert len(set(zip(pend["conn"].tolist(), pend["xid"].tolist()))) < len(pend)


def _reply_batch(replies_, payload=None):
    pay = np.zeros(1, np.uint8) if payload is None else payload
    return L.HostBatch(np.ascontiguousarray(replies_), np.zeros(1, L.UNIX_DTYPE), np.zeros(1, np.uint8), pay)


def test_end_to_end_300_records(R, codec):
    import route_model as RM
    nh, nconn = 4, 3
    tab = RM.table([(100003, 3, 0, 4, 0, 0), (100003, 4, 0, 2, 0, 1), (100005, 3, 0, 6, 1, 1)])
    rng = np.random.default_rng(41)
    msgs = [d for d in S.random_messages(900, seed=41, max_payload=200) if d["type"] == "call"][:300]
    assert len(msgs) == 300
    progs = [(100003, 3), (100003, 4), (100005, 3), (100003, 2), (100021, 4)]
    for i, d in enumerate(msgs):
        d["xid"] = 0xFFFFF000 + i if i % 2 else (i * 2654435761) & TOP        # all different, some past 2^31
        d["program"], d["program_version"] = progs[int(rng.integers(0, len(progs)))]
        d["procedure"] = int(rng.integers(0, 8))
    assert len({d["xid"] for d in msgs}) == 300
    call_conn = rng.integers(0, nconn, 300).astype(np.uint32)      # the connection each Call goes out on
    # 1. the Calls encoded, decoded, routed
    wire, off, st, _ = R.encode_host_batch(codec, L.build_batch(msgs))
    assert not st.any()
    w = np.frombuffer(wire + b"\0" * 16, np.uint8).copy()
    dm, _, ds, _, _ = R.decode_host_wire(codec, w, off, L.DECODE_SLICE)
    assert not ds.any() and dm["xid"].tolist() == [d["xid"] for d in msgs]
    g = R.route_calls_host(codec, dm, ds, tab, nh)
    first = g["bin_first"].astype(np.int64)
    assert int(g["result"][0]) > 30 and int(g["result"][1]) > 30 and int(g["result"][2]) == 0
    # 2. the rejected slice as it stands and the handlers' slices with payloads filled in, encoded
    rep = g["replies"].copy()
    arena = rng.integers(0, 256, 64 * 300, dtype=np.uint8)
    served = np.arange(int(first[nh]))
    rep["payload_off"][served] = 64 * served
    rep["payload_len"][served] = rng.integers(0, 65, len(served))
    r_wire, r_off, r_st, _ = R.encode_host_batch(codec, _reply_batch(rep, arena))
    assert not r_st.any() and len(r_off) == 301
    # 3. the reply stream cut into per-connection segments: a Reply travels on its Call's connection
    conn_of = call_conn[g["order"]]                  # reply k answers Call order[k]
    slab, seg_off, seg_len, arrival = bytearray(), [], [], []
    for c in (2, 0, 1):
        slab += b"\xEE" * (11 + 5 * c)
        seg_off.append(len(slab))
        mine = np.flatnonzero(conn_of == c)
        for k in mine:
            slab += r_wire[int(r_off[k]):int(r_off[k + 1])]
        seg_len.append(len(slab) - seg_off[-1])
        arrival += [(c, int(k)) for k in mine]
    seg_conn = np.array([2, 0, 1], np.uint32)
    tags = np.arange(300, dtype=np.uint64)
    pend = np.zeros(300, L.PENDING_DTYPE)
    pend["conn"], pend["xid"], pend["tag"] = call_conn, dm["xid"], tags

    def receive(segs):
        # 4. framed and decoded with rec_seg; 5. matched with rec_conn = the segments' connections
        so, sl = [seg_off[s] for s in segs], [seg_len[s] for s in segs]
        rec_start, rec_len, rec_seg, _, res = R.frame_host_streams(codec, bytes(slab), so, sl)
        sw = np.frombuffer(bytes(slab) + b"\0" * 16, np.uint8).copy()
        rm, _, rs, _, _ = R.decode_host_extents(codec, sw, rec_start, rec_len, L.DECODE_SLICE, wire_len=len(slab))
        assert not rs.any() and (rm["msg_type"] == L.MSG_REPLY).all()
        rec_conn = seg_conn[np.array(segs)][rec_seg]
        want = _check(R, codec, rm, rs, rec_conn, pend, f"end to end, segments {segs}")
        return rm, rec_conn, want

    rm, rec_conn, want = receive([0, 1, 2])
    assert len(rm) == 300 and [(int(c), int(x)) for c, x in zip(rec_conn, rm["xid"])] == \
        [(c, int(rep["xid"][k])) for c, k in arrival]
    # 6. every entry hit exactly once, tag_out names the Call whose xid the Reply carries, still is empty
    assert want["result"].tolist() == [300, 0, 0, 0, 0, 0] and len(want["still"]) == 0
    assert sorted(want["hit"].tolist()) == list(range(300))
    call_xid = dm["xid"][want["tag_out"].astype(np.int64)]
    assert np.array_equal(call_xid, rm["xid"]) and np.array_equal(call_conn[want["tag_out"].astype(np.int64)], rec_conn)
    # ... and without connection 0's segment exactly its Calls are left
    rm, rec_conn, want = receive([0, 2])
    assert want["still"]["tag"].tolist() == np.flatnonzero(call_conn == 0).tolist()
    assert int(want["result"][0]) == len(rm) == 300 - int((call_conn == 0).sum())


def test_mapped_host_memory(R, codec):
    import torch
    n, npend = 2 * T + 9, T + 70
    m, status, rc, pend = _mixed_case(n, npend, 5, False)
    want = M.match(m, status, rc, pend)
    k = len(want["still"])
    h_msgs = R.HostMapped.from_array(codec, m)
    h_pend = R.HostMapped.from_array(codec, pend)
    h_match = R.HostMapped.from_array(codec, np.full(4 * (n + 4), SENT, np.uint8))
    h_hit = R.HostMapped.from_array(codec, np.full(4 * (npend + 4), SENT, np.uint8))
    h_still = R.HostMapped.from_array(codec, np.full(16 * (npend + 4), SENT, np.uint8))
    try:
        d_st = torch.from_numpy(status.copy()).cuda()
        d_rc = torch.from_numpy(rc.view(np.int32).copy()).cuda()
        tag = torch.full((n + 4,), -1, dtype=torch.int64, device="cuda")
        res = torch.full((7,), -1, dtype=torch.int64, device="cuda")
        codec.match_replies(h_msgs, d_st, d_rc, n, h_pend, npend, h_match, h_hit, res, tag_out=tag, still=h_still)
        codec.sync()
        assert res.cpu().numpy().view(np.uint64).tolist() == want["result"].tolist() + [2**64 - 1]
        assert np.array_equal(h_match.view(np.uint32)[:n], want["match"]) and (h_match.view(np.uint32)[n:] == S32).all()
        assert np.array_equal(h_hit.view(np.uint32)[:npend], want["hit"]) and (h_hit.view(np.uint32)[npend:] == S32).all()
        assert h_still.host[:16 * k].tobytes() == want["still"].tobytes() and (h_still.host[16 * k:] == SENT).all()
        assert np.array_equal(tag.cpu().numpy().view(np.uint64)[:n], want["tag_out"]) and tag[n].item() == -1
        assert h_msgs.host.tobytes() == m.tobytes() and h_pend.host.tobytes() == pend.tobytes()
    finally:
        for h in (h_msgs, h_pend, h_match, h_hit, h_still):
            h.close()


def test_graph_capture_and_replay(R):
    import torch
    n, npend = 2 * T + 77, 2 * T + 5
    d_msgs = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_rc = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_pend = torch.zeros(npend * 16, dtype=torch.uint8, device="cuda")
    match = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    hit = torch.full((npend + 1,), -1, dtype=torch.int32, device="cuda")
    tag = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    still = torch.full(((npend + 1) * 16,), SENT, dtype=torch.uint8, device="cuda")
    res = torch.full((7,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def work(codec):
        codec.match_replies(d_msgs, d_st, d_rc, n, d_pend, npend, match, hit, res, tag_out=tag, still=still)

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
        assert (match == -1).all().item() and (res == -1).all().item() and (still == SENT).all().item()
        codec.reserve(max(n, npend))
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            work(codec)                              # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            work(codec)
        torch.cuda.synchronize()
        for seed in (5, 6, 7):
            m, st, rc, pend = _mixed_case(n, npend, seed, False)
            if seed == 7:                            # the list shrunk to nothing that is hit: all NONE
                pend["conn"] += 100
            d_msgs.copy_(torch.from_numpy(m.view(np.uint8).reshape(-1).copy()).cuda())
            d_st.copy_(torch.from_numpy(st.copy()).cuda())
            d_rc.copy_(torch.from_numpy(rc.view(np.int32).copy()).cuda())
            d_pend.copy_(torch.from_numpy(pend.view(np.uint8).reshape(-1).copy()).cuda())
            for t in (match, hit, tag, res):
                t.fill_(-1)
            still.fill_(SENT)
            g.replay()
            torch.cuda.synchronize()
            want = M.match(m, st, rc, pend)
            k = len(want["still"])
            assert res.cpu().numpy().view(np.uint64).tolist() == want["result"].tolist() + [2**64 - 1]
            assert np.array_equal(match.cpu().numpy().view(np.uint32)[:n], want["match"])
            assert np.array_equal(hit.cpu().numpy().view(np.uint32)[:npend], want["hit"])
            assert np.array_equal(tag.cpu().numpy().view(np.uint64)[:n], want["tag_out"])
            assert still.cpu().numpy()[:16 * k].tobytes() == want["still"].tobytes()
            assert (still.cpu().numpy()[16 * k:] == SENT).all()
            assert match[n].item() == -1 and hit[npend].item() == -1 and tag[n].item() == -1
            if seed == 7:
                assert k == npend and (want["hit"] == M.NONE).all() and int(want["result"][0]) == 0
    finally:
        fresh.close()
        codec.close()


def test_cpp_mirror(R, codec, tmp_path, oracle):
    """PendingCalls / match_replies / MatchedReplies of include/onc_rpc.hpp
    (tests/cpp_match/test_match.cpp) over a wire, its records' connections and
    a list written here; both of its rounds are compared with the model's."""
    exe = os.path.join(ROOT, "tests", "cpp_match", "test_match")
    assert os.path.exists(exe), "build() compiles tests/cpp_match"
    rng = np.random.default_rng(12)
    msgs = S.random_messages(200, seed=5, max_payload=64)
    for i, d in enumerate(msgs):
        d["xid"] = 1000 + i % 120                     # (xids repeat: duplicates, and the same xid on two connections)
    wire, off, st, _ = oracle.encode_batch(L.build_batch(msgs))
    assert not st.any()
    conns = rng.integers(0, 3, 200).astype(np.uint32)
    conns[120:] = conns[:80]                          # (... and on the same one: a duplicate where both are Replies)
    # the list: three of every four records' keys, whatever they are, then keys nobody answers
    rows = [(int(conns[i]), 1000 + i % 120, int(rng.integers(0, 1 << 63))) for i in range(120) if i % 4]
    rows += [(int(rng.integers(0, 3)), 2000 + i, i) for i in range(40)]
    rows[7] = rows[3]                                 # a repeated key: answered in the second round
    pend = M.pending(rows)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<QQQ", len(pend), 200, len(wire)))
        f.write(pend.tobytes())
        f.write(conns.tobytes())
        f.write(wire)
    r = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASS test_match" in r.stdout, r.stdout + r.stderr
    w = np.frombuffer(wire + b"\0" * 16, np.uint8).copy()
    dm, _, ds, _, _ = oracle.decode_batch(w, off, L.DECODE_SLICE)
    blob, at = open(outp, "rb").read(), 0
    for rnd in range(2):
        want = M.match(dm, ds, conns, pend)
        n, npend = struct.unpack_from("<QQ", blob, at)
        assert (n, npend) == (200, len(pend))
        at += 16
        match = np.frombuffer(blob, np.uint32, n, at)
        at += 4 * n
        tag = np.frombuffer(blob, np.uint64, n, at)
        at += 8 * n
        hit = np.frombuffer(blob, np.uint32, npend, at)
        at += 4 * npend
        res = np.frombuffer(blob, np.uint64, 6, at)
        at += 48
        still = np.frombuffer(blob, L.PENDING_DTYPE, int(res[5]), at)
        at += 16 * int(res[5])
        assert np.array_equal(match, want["match"]) and np.array_equal(tag, want["tag_out"]), f"round {rnd}"
        assert np.array_equal(hit, want["hit"]) and res.tolist() == want["result"].tolist(), f"round {rnd}"
        assert still.tobytes() == want["still"].tobytes(), f"round {rnd}"
        if rnd == 0:
            assert int(res[0]) > 20 and int(res[2]) > 0 and int(res[3]) > 0 and int(res[1]) > 0
        pend = want["still"]
    assert at == len(blob)
