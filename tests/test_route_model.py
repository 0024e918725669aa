"""tests/route_model.py (the expected value of every onc_route_calls test)
against hand-written cases: each outcome of the lookup and each rule of the
table."""
import numpy as np

import onc_rpc_amd.layout as L
import route_model as M

NFS, MOUNT = 100003, 100005
# nh = 6: NFS v3 procedures 0..2 -> handlers 0..2, 4..5 -> handler 3 (one handler), NFS v4 -> 4, MOUNT v3 0 -> 5
TAB = M.table([(NFS, 3, 0, 3, 0, 0), (NFS, 3, 4, 2, 3, 1), (NFS, 4, 0, 2, 4, 1), (MOUNT, 3, 0, 1, 5, 0)])
NH = 6


def test_lookup_outcomes():
    assert M.first_bad(TAB, NH) == 0
    assert M.lookup(TAB, NH, NFS, 3, 0) == (0, 0, 0, 0)
    assert M.lookup(TAB, NH, NFS, 3, 2) == (2, 0, 0, 0)
    assert M.lookup(TAB, NH, NFS, 3, 3) == (NH, M.PROC_UNAVAIL, 0, 0)          # the gap
    assert M.lookup(TAB, NH, NFS, 3, 4) == (3, 0, 0, 0)
    assert M.lookup(TAB, NH, NFS, 3, 5) == (3, 0, 0, 0)                        # one handler for the range
    assert M.lookup(TAB, NH, NFS, 3, 6) == (NH, M.PROC_UNAVAIL, 0, 0)
    assert M.lookup(TAB, NH, NFS, 4, 1) == (4, 0, 0, 0)
    assert M.lookup(TAB, NH, NFS, 2, 0) == (NH, M.PROG_MISMATCH, 3, 4)
    assert M.lookup(TAB, NH, NFS, 5, 0) == (NH, M.PROG_MISMATCH, 3, 4)
    assert M.lookup(TAB, NH, MOUNT, 1, 0) == (NH, M.PROG_MISMATCH, 3, 3)       # a single version: low == high
    assert M.lookup(TAB, NH, MOUNT, 3, 1) == (NH, M.PROC_UNAVAIL, 0, 0)
    assert M.lookup(TAB, NH, 100000, 3, 0) == (NH, M.PROG_UNAVAIL, 0, 0)
    assert M.lookup(TAB, NH, 0xFFFFFFFF, 3, 0) == (NH, M.PROG_UNAVAIL, 0, 0)
    assert M.lookup(M.table([]), 0, NFS, 3, 0) == (0, M.PROG_UNAVAIL, 0, 0)


def test_table_rules():
    ok = [(1, 1, 0, 2, 0, 0), (1, 1, 2, 2, 2, 0), (1, 2, 0, 4, 0, 0), (2, 0, 0, 1, 3, 0)]
    assert M.first_bad(M.table(ok), 4) == 0
    assert M.first_bad(M.table(ok), 3) == 2                    # handler_first + proc_count > nh
    assert M.first_bad(M.table([]), 0) == 0
    assert M.first_bad(M.table([(1, 1, 0, 1, 0, 0)]), 0) == 1  # nh == 0: only the empty table

    def bad(i, row, nh=4):
        rows = list(ok)
        rows[i] = row
        return M.first_bad(M.table(rows), nh)

    assert bad(1, (1, 1, 2, 0, 2, 0)) == 2                     # proc_count == 0
    assert bad(3, (2, 0, 0xFFFFFFFF, 2, 0, 1)) == 4            # proc_first + proc_count > 2^32
    assert bad(3, (2, 0, 0xFFFFFFFF, 1, 3, 0)) == 0            # ... == 2^32
    assert bad(3, (2, 0, 0, 0xFFFFFFFF, 3, 1)) == 0            # ONE_HANDLER: one handler whatever the count
    assert bad(3, (2, 0, 0, 0xFFFFFFFF, 4, 1)) == 4
    assert bad(2, (1, 2, 0, 4, 0, 2)) == 3                     # an unknown flag
    assert bad(0, (1, 1, 0, 3, 0, 0)) == 1                     # ranges of one (program, version) overlap: the pair's first
    assert bad(1, (1, 1, 0, 2, 2, 0)) == 1                     # equal keys
    assert bad(2, (1, 0, 0, 4, 0, 0)) == 2                     # version descends: pair (1, 2)
    assert bad(3, (0, 9, 9, 1, 3, 0)) == 3                     # program descends: pair (2, 3)
    assert bad(1, (1, 1, 1, 1, 2, 0)) == 1                     # in order, but inside the range before it
    assert bad(0, (1, 1, 3, 1, 0, 0)) == 1                     # out of order only in the third key word
    # the first bad entry wins, and an entry's own rule comes before its pair's
    rows = [(5, 5, 5, 0, 0, 0), (1, 1, 1, 0, 0, 0)]
    assert M.first_bad(M.table(rows), 4) == 1
    # unsigned: 0x80000000 sorts after 0x7FFFFFFF
    assert M.first_bad(M.table([(0x7FFFFFFF, 0, 0, 1, 0, 0), (0x80000000, 0, 0, 1, 0, 0)]), 1) == 0
    assert M.first_bad(M.table([(0x80000000, 0, 0, 1, 0, 0), (0x7FFFFFFF, 0, 0, 1, 0, 0)]), 1) == 1


def test_route_calls_groups_and_replies():
    keys = [(NFS, 3, 1), (7, 7, 7), (NFS, 3, 0), (NFS, 9, 0), (NFS, 3, 1), (MOUNT, 3, 5), (NFS, 3, 5)]
    msgs = np.concatenate([M.calls(keys, xid0=100), np.zeros(3, L.MSG_DTYPE)])
    msgs[7]["msg_type"], msgs[7]["xid"] = L.MSG_REPLY, 55      # a client's Reply
    msgs[8]["msg_type"] = 7                                     # not a message type: still not a Call
    msgs[9]["f0"] = NFS                                         # failed: never looked at
    status = np.array([0] * 9 + [3], np.int32)
    msgs[0]["payload_off"], msgs[0]["payload_len"], msgs[0]["cred_ref"] = (1 << 40) + 3, 77, 12345
    out = M.route_calls(msgs, status, TAB, NH)
    assert out["route"].tolist() == [1, NH, 0, NH, 1, NH, 3, NH + 1, NH + 1, NH + 2]
    assert out["order"].tolist() == [2, 0, 4, 6, 1, 3, 5, 7, 8, 9]
    assert out["bin_first"].tolist() == [0, 1, 3, 3, 4, 4, 4, 7, 9, 10]
    assert out["result"].tolist() == [4, 3, 3, 0]
    assert out["calls_out"].tobytes() == msgs[out["order"]].tobytes()
    rep = out["replies"]
    assert rep["xid"].tolist() == [102, 100, 104, 106, 101, 103, 105, 0, 0, 0]
    assert rep["msg_type"][:7].tolist() == [1] * 7 and rep["reply_stat"].tolist() == [0] * 10
    assert rep["stat"].tolist() == [0, 0, 0, 0, M.PROG_UNAVAIL, M.PROG_MISMATCH, M.PROC_UNAVAIL, 0, 0, 0]
    assert (rep["f0"][5], rep["f1"][5], rep["f2"][5]) == (3, 4, 0)
    assert not rep[7:].tobytes().strip(b"\0")                   # no reply for what is not an OK Call
    for f in ("payload_len", "payload_off", "cred_id", "cred_kind_len", "cred_ref", "verf_id", "verf_kind_len",
              "verf_ref", "auth_stat"):
        assert not rep[f].any(), f
    assert not np.delete(rep["f0"], 5).any() and not np.delete(rep["f1"], 5).any() and not rep["f2"].any()

    bad = M.route_calls(msgs, status, M.table([(1, 1, 0, 0, 0, 0)]), NH)
    assert bad["result"].tolist() == [0, 0, 0, 1] and bad["bin_first"].tolist() == [0] * (NH + 4)
    assert bad["route"] is None and bad["order"] is None and bad["replies"] is None

    none = M.route_calls(msgs[:0], status[:0], TAB, NH)
    assert none["result"].tolist() == [0, 0, 0, 0] and none["bin_first"].tolist() == [0] * (NH + 4)
    empty = M.route_calls(msgs, status, M.table([]), 0)         # every Call PROG_UNAVAIL
    assert empty["route"].tolist() == [0] * 7 + [1, 1, 2] and empty["result"].tolist() == [0, 7, 3, 0]


def _same_result(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        if a[k] is None:
            assert b[k] is None, k
        else:
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_the_fast_form_is_the_loop():
    """route_calls_fast (the expected value of the batches of hundreds of
    thousands of records in tests/test_gpu_scan_rounds.py) == route_calls on
    the cases above and on a batch with every outcome mixed."""
    keys = [(NFS, 3, 1), (7, 7, 7), (NFS, 3, 0), (NFS, 9, 0), (NFS, 3, 1), (MOUNT, 3, 5), (NFS, 3, 5)]
    msgs = np.concatenate([M.calls(keys, xid0=100), np.zeros(3, L.MSG_DTYPE)])
    msgs[7]["msg_type"], msgs[7]["xid"] = L.MSG_REPLY, 55
    msgs[8]["msg_type"] = 7
    msgs[9]["f0"] = NFS
    status = np.array([0] * 9 + [3], np.int32)
    for tab, nh in ((TAB, NH), (M.table([(1, 1, 0, 0, 0, 0)]), NH), (M.table([]), 0)):
        _same_result(M.route_calls_fast(msgs, status, tab, nh), M.route_calls(msgs, status, tab, nh))
    _same_result(M.route_calls_fast(msgs[:0], status[:0], TAB, NH), M.route_calls(msgs[:0], status[:0], TAB, NH))
    rng = np.random.default_rng(5)
    n = 3000
    m = np.frombuffer(rng.bytes(64 * n), L.MSG_DTYPE).copy()
    st = np.where(rng.integers(0, 5, n) == 0, rng.choice((1, 10, 106, -3), n), 0).astype(np.int32)
    m["msg_type"] = rng.choice((L.MSG_CALL, L.MSG_CALL, L.MSG_CALL, L.MSG_REPLY, 7), n)
    m["f0"] = rng.choice((NFS, NFS, MOUNT, 100000, 0xFFFFFFFF), n)
    m["f1"] = rng.choice((3, 3, 4, 2, 0xFFFFFFFF), n)
    m["f2"] = rng.integers(0, 8, n)
    want = M.route_calls(m, st, TAB, NH)
    assert (np.bincount(want["route"], minlength=NH + 3) > 0).all() and set(want["stat"].tolist()) == {0, 1, 2, 3}
    _same_result(M.route_calls_fast(m, st, TAB, NH), want)
