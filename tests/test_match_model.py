"""tests/match_model.py (the expected value of every onc_match_replies test)
pinned by cases written out by hand from the contract in include/onc_rpc.h."""
import numpy as np

import match_model as M
import onc_rpc_amd.layout as L

U, D, NR, F, NONE = M.UNKNOWN, M.DUPLICATE, M.NOT_REPLY, M.FAILED, M.NONE


def _run(xids, conns, rows, status=None, msg_type=None):
    msgs = M.replies(xids)
    if msg_type is not None:
        msgs["msg_type"] = np.asarray(msg_type, np.uint8)
    st = np.zeros(len(xids), np.int32) if status is None else np.asarray(status, np.int32)
    rc = None if conns is None else np.asarray(conns, np.uint32)
    return M.match(msgs, st, rc, M.pending(rows))


def _same(got, match, hit, tag, still, result):
    assert got["match"].tolist() == match
    assert got["hit"].tolist() == hit
    assert got["tag_out"].tolist() == tag
    assert [tuple(int(x) for x in e) for e in got["still"]] == still
    assert got["result"].tolist() == result
    assert got["match"].dtype == np.uint32 and got["hit"].dtype == np.uint32
    assert got["tag_out"].dtype == np.uint64 and got["result"].dtype == np.uint64
    assert got["still"].dtype == L.PENDING_DTYPE


def test_constants():
    assert (U, D, NR, F, NONE, M.MAX, M.TILE) == (0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC, 0xFFFFFFFF,
                                                  0xFFFFFFF0, 1024)
    assert L.PENDING_DTYPE.itemsize == 16 and L.MSG_REPLY == 1


def test_same_xid_on_two_connections():
    rows = [(1, 7, 100), (2, 7, 200), (3, 8, 300)]
    got = _run([7, 7, 7], [2, 1, 3], rows)
    _same(got, [1, 0, U], [1, 0, NONE], [200, 100, 0], [(3, 8, 300)], [2, 1, 0, 0, 0, 1])


def test_rec_conn_null_is_connection_zero():
    rows = [(0, 5, 50), (1, 5, 51), (0, 6, 60)]
    got = _run([5, 6, 5], None, rows)
    _same(got, [0, 2, D], [0, NONE, 1], [50, 60, 0], [(1, 5, 51)], [2, 0, 1, 0, 0, 1])


def test_no_reserved_key():
    T = 0xFFFFFFFF
    rows = [(T, T, 1), (0, 0, 2), (T, 0, 3), (0, T, 4)]
    got = _run([0, T, 0, T, 1], [0, T, T, 0, 0], rows)
    _same(got, [1, 0, 2, 3, U], [1, 0, 2, 3], [2, 1, 3, 4, 0], [], [4, 1, 0, 0, 0, 0])


def test_key_repeated_three_times_over_three_calls():
    rows = [(4, 9, 11), (5, 1, 99), (4, 9, 22), (4, 9, 33)]
    g1 = _run([9], [4], rows)
    _same(g1, [0], [0, NONE, NONE, NONE], [11], [(5, 1, 99), (4, 9, 22), (4, 9, 33)], [1, 0, 0, 0, 0, 3])
    g2 = M.match(M.replies([9]), np.zeros(1, np.int32), np.array([4], np.uint32), g1["still"])
    _same(g2, [1], [NONE, 0, NONE], [22], [(5, 1, 99), (4, 9, 33)], [1, 0, 0, 0, 0, 2])
    g3 = M.match(M.replies([9]), np.zeros(1, np.int32), np.array([4], np.uint32), g2["still"])
    _same(g3, [1], [NONE, 0], [33], [(5, 1, 99)], [1, 0, 0, 0, 0, 1])
    g4 = M.match(M.replies([9]), np.zeros(1, np.int32), np.array([4], np.uint32), g3["still"])
    _same(g4, [U], [NONE], [0], [(5, 1, 99)], [0, 1, 0, 0, 0, 1])


def test_three_replies_to_one_call():
    rows = [(0, 1, 10), (0, 2, 20)]
    got = _run([3, 2, 2, 1, 2], [0] * 5, rows)
    _same(got, [U, 1, D, 0, D], [3, 1], [0, 20, 0, 10, 0], [], [2, 1, 2, 0, 0, 0])


def test_failed_record_is_not_looked_at():
    rows = [(0, 1, 10)]
    # record 0 failed: its descriptor says Reply, xid 1, connection 0 — and does not answer
    got = _run([1, 1], [0, 0], rows, status=[-3, 0])
    _same(got, [F, 0], [1], [0, 10], [], [1, 0, 0, 0, 1, 0])
    got = _run([1], [0], rows, status=[7])
    _same(got, [F], [NONE], [0], [(0, 1, 10)], [0, 0, 0, 0, 1, 1])


def test_msg_types_other_than_reply():
    rows = [(0, 1, 10)]
    got = _run([1, 1, 1], [0, 0, 0], rows, msg_type=[0, 7, 1])
    _same(got, [NR, NR, 0], [2], [0, 0, 10], [], [1, 0, 0, 2, 0, 0])


def test_no_pending_entries():
    got = _run([1, 2, 3], [0, 0, 0], [], status=[0, 1, 0], msg_type=[1, 1, 0])
    _same(got, [U, F, NR], [], [0, 0, 0], [], [0, 1, 0, 1, 1, 0])


def test_no_records():
    rows = [(1, 2, 3), (1, 2, 4)]
    got = _run([], [], rows)
    _same(got, [], [NONE, NONE], [], [(1, 2, 3), (1, 2, 4)], [0, 0, 0, 0, 0, 2])
    got = _run([], None, [])
    _same(got, [], [], [], [], [0, 0, 0, 0, 0, 0])


def test_the_fast_form_is_the_loop():
    """match_fast (the expected value of the lists and batches of a million
    entries in tests/test_gpu_scan_rounds.py) == match on the cases above and
    on a batch with every outcome mixed, keys repeated in the list and in the
    batch."""
    def same(msgs, st, rc, pend):
        a, b = M.match_fast(msgs, st, rc, pend), M.match(msgs, st, rc, pend)
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        return b

    T = 0xFFFFFFFF
    hand = [([7, 7, 7], [2, 1, 3], [(1, 7, 100), (2, 7, 200), (3, 8, 300)]),
            ([5, 6, 5], None, [(0, 5, 50), (1, 5, 51), (0, 6, 60)]),
            ([0, T, 0, T, 1], [0, T, T, 0, 0], [(T, T, 1), (0, 0, 2), (T, 0, 3), (0, T, 4)]),
            ([9], [4], [(4, 9, 11), (5, 1, 99), (4, 9, 22), (4, 9, 33)]),
            ([3, 2, 2, 1, 2], [0] * 5, [(0, 1, 10), (0, 2, 20)]),
            ([1, 2, 3], [0, 0, 0], []), ([], [], [(1, 2, 3), (1, 2, 4)]), ([], None, [])]
    for xids, conns, rows in hand:
        rc = None if conns is None else np.asarray(conns, np.uint32)
        same(M.replies(xids), np.zeros(len(xids), np.int32), rc, M.pending(rows))
    rng = np.random.default_rng(3)
    n, npend = 4000, 1500
    pend = np.zeros(npend, L.PENDING_DTYPE)
    pend["conn"], pend["xid"] = rng.integers(0, 3, npend), rng.integers(0, 900, npend)
    pend["tag"] = rng.integers(0, 1 << 64, npend, dtype=np.uint64)
    msgs = np.frombuffer(rng.bytes(64 * n), L.MSG_DTYPE).copy()
    msgs["xid"] = rng.integers(0, 1400, n)
    msgs["msg_type"] = rng.choice((L.MSG_REPLY, L.MSG_REPLY, L.MSG_REPLY, L.MSG_CALL, 7), n)
    st = np.where(rng.integers(0, 6, n) == 0, 106, 0).astype(np.int32)
    rc = rng.integers(0, 3, n).astype(np.uint32)
    want = same(msgs, st, rc, pend)
    assert (want["result"] > 0).all() and len(set(zip(pend["conn"].tolist(), pend["xid"].tolist()))) < npend
    same(msgs, st, None, pend)
