"""tests/group_model.py against the contract of onc_group_by_conn written out as
a plain loop: short lists of every size up to 20, with and without via, via
entries at and past nsrc, connection ids at nconn - 1, nconn, nconn + 1 and
0xFFFFFFFF; and conn_extents with nrec below, at and above conn_first[nconn]."""
import numpy as np

import group_model as M


def _same(rec_conn, via, nconn):
    got = M.group(rec_conn, via, nconn)
    order, conn_first, result = M.brute(rec_conn, via, nconn)
    assert got["order"].tolist() == order, (rec_conn, via, nconn)
    assert got["conn_first"].tolist() == conn_first
    assert got["result"].tolist() == result
    assert got["order"].dtype == np.uint32 and got["conn_first"].dtype == np.uint64


def test_model_against_the_loop_every_size_up_to_20():
    rng = np.random.default_rng(11)
    for n in range(21):
        for nconn in (0, 1, 2, 3, 7):
            edge = [max(nconn - 1, 0), nconn, nconn + 1, 0xFFFFFFFF]
            rc = [int(rng.integers(0, nconn + 1)) if rng.random() < 0.7 else edge[int(rng.integers(0, 4))]
                  for _ in range(n)]
            _same(rc, None, nconn)
            for m in (0, 1, n, n + 3):
                via = [int(rng.integers(0, max(n, 1))) for _ in range(m)]
                _same(rc, via, nconn)
                # entries at nsrc, past it and at 0xFFFFFFFF: dropped, never read
                if m >= 3:
                    via[0], via[m // 2], via[m - 1] = n, n + 1, 0xFFFFFFFF
                    _same(rc, via, nconn)


def test_model_edges():
    # every key at an edge
    for nconn in (1, 2, 5):
        rc = [nconn - 1, nconn, nconn + 1, 0xFFFFFFFF, 0, nconn - 1, 0xFFFFFFFF, 0]
        _same(rc, None, nconn)
        got = M.group(rc, None, nconn)
        assert got["result"].tolist() == [4, 4, 1 if nconn == 1 else 2]
    # nconn == 0: everything is group 0 and the order is the identity
    got = M.group([5, 0, 9], None, 0)
    assert got["order"].tolist() == [0, 1, 2] and got["conn_first"].tolist() == [0, 3] and got["result"].tolist() == [0, 3, 0]
    # no items
    got = M.group([], None, 3)
    assert got["order"].tolist() == [] and got["conn_first"].tolist() == [0] * 5 and got["result"].tolist() == [0, 0, 0]
    # descriptors follow the order
    got = M.group([2, 0, 2, 1], None, 3, msgs=np.array([10, 11, 12, 13]))
    assert got["msgs_out"].tolist() == [11, 13, 10, 12]
    assert (M.bits(0), M.bits(1), M.bits(255), M.bits(256)) == (0, 1, 8, 9)
    assert [M.passes(x) for x in (0, 1, 255, 256, 65535, 65536, M.CONN_MAX)] == [0, 1, 1, 2, 2, 3, 3]


def test_conn_extents_clamp():
    rec_off = np.array([0, 10, 30, 60, 100, 150], np.uint64)         # 5 records
    g = M.group([1, 9, 0, 1, 9], None, 3)                            # sent 3, dropped 2
    cf = g["conn_first"]
    assert cf.tolist() == [0, 1, 3, 3, 5] and int(g["result"][0]) == 3
    # nrec above conn_first[nconn]: the whole batch was encoded
    assert M.conn_extents(rec_off, 5, cf).tolist() == [0, 10, 60, 60, 150]
    # at it: only the sent records were encoded; the dropped group's range is empty
    assert M.conn_extents(rec_off[:4], 3, cf).tolist() == [0, 10, 60, 60, 60]
    # below it: everything from record 2 on reads rec_off[2]
    assert M.conn_extents(rec_off[:3], 2, cf).tolist() == [0, 10, 30, 30, 30]
    assert M.conn_extents(rec_off[:1], 0, cf).tolist() == [0] * 5
