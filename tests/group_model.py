"""The host model of onc_group_by_conn and onc_conn_extents (include/onc_rpc.h):
numpy's stable argsort of the clamped keys and searchsorted for conn_first.
brute() is the header's pseudocode as a plain Python loop, for
tests/test_group_model.py to hold the model against."""
import numpy as np

TILE = 1024
CONN_MAX = 0x00FFFFFF


def bits(nconn):
    return int(nconn).bit_length()


def passes(nconn):
    return (bits(nconn) + 7) // 8


def keys(rec_conn, via, nconn, n=None):
    """key[k] = min(rec_conn[via[k]], nconn); an index outside rec_conn: nconn."""
    rc = np.asarray(rec_conn, np.uint64)
    s = np.arange(len(rc) if n is None else n, dtype=np.uint64) if via is None else np.asarray(via, np.uint64)
    inside = s < len(rc)
    c = np.full(len(s), nconn, np.uint64)
    if len(rc):
        c[inside] = rc[s[inside]]
    return np.minimum(c, np.uint64(nconn))


def group(rec_conn, via, nconn, msgs=None):
    """-> dict(order[n] u32, conn_first[nconn + 2] u64, result[3] u64, msgs_out or None)."""
    key = keys(rec_conn, via, nconn)
    order = np.argsort(key, kind="stable").astype(np.uint32)
    conn_first = np.searchsorted(key[order], np.arange(nconn + 2, dtype=np.uint64), side="left").astype(np.uint64)
    n = len(key)
    sent = int(conn_first[nconn])
    active = int(np.count_nonzero(np.diff(conn_first[:nconn + 1])))
    return {"order": order, "conn_first": conn_first, "result": np.array([sent, n - sent, active], np.uint64),
            "msgs_out": None if msgs is None else np.asarray(msgs)[order]}


def conn_extents(rec_off, nrec, conn_first):
    """conn_off[c] = rec_off[min(conn_first[c], nrec)]."""
    ro = np.asarray(rec_off, np.uint64)
    return ro[np.minimum(np.asarray(conn_first, np.uint64), np.uint64(nrec)).astype(np.int64)]


def brute(rec_conn, via, nconn):
    """The contract, item by item -> (order, conn_first, result) as lists."""
    n = len(rec_conn) if via is None else len(via)
    key = []
    for k in range(n):
        s = k if via is None else int(via[k])
        c = int(rec_conn[s]) if s < len(rec_conn) else nconn
        key.append(min(c, nconn))
    order = []
    for c in range(nconn + 1):
        order += [k for k in range(n) if key[k] == c]
    conn_first = [sum(1 for k in range(n) if key[k] < c) for c in range(nconn + 2)]
    active = sum(1 for c in range(nconn) if any(key[k] == c for k in range(n)))
    return order, conn_first, [conn_first[nconn], n - conn_first[nconn], active]
