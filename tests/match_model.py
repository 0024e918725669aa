"""onc_match_replies restated in numpy / plain Python from the pseudocode of
include/onc_rpc.h: the expected value of every match test. The lead of a key
comes from a Python dict filled in list order and the duplicates from a set of
leads seen so far, in record order — no slot table, no probing, no atomics —
so that it does not share the kernels' bug class. Pure host logic."""
import numpy as np

import onc_rpc_amd.layout as L

UNKNOWN, DUPLICATE, NOT_REPLY, FAILED = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC
NONE = 0xFFFFFFFF
MAX = 0xFFFFFFF0
TILE = 1024
ONE_CHAIN = 0x80000


def pending(rows):
    """(conn, xid, tag) rows, as given."""
    t = np.zeros(len(rows), L.PENDING_DTYPE)
    for i, row in enumerate(rows):
        t[i] = tuple(row)
    return t


def replies(xids, msg_type=L.MSG_REPLY):
    """Reply descriptors that carry the xids and nothing else."""
    m = np.zeros(len(xids), L.MSG_DTYPE)
    m["xid"] = np.asarray(xids, np.uint32)
    m["msg_type"] = msg_type
    return m


def leads(pend):
    """{(conn, xid): the lowest index with that key}."""
    lead = {}
    for p in range(len(pend)):
        lead.setdefault((int(pend["conn"][p]), int(pend["xid"][p])), p)
    return lead


def match(msgs, status, rec_conn, pend):
    """The whole result: a dict of match[n], hit[np], tag_out[n], still[k] and
    result[6] (tag_out and still as a call that asks for them writes them)."""
    n, npend = len(msgs), len(pend)
    lead = leads(pend)
    out = np.zeros(n, np.uint32)
    hit = np.full(npend, NONE, np.uint32)
    tag = np.zeros(n, np.uint64)
    seen = set()
    xid, mt = msgs["xid"], msgs["msg_type"]
    for r in range(n):
        if int(status[r]) != 0:
            out[r] = FAILED
        elif int(mt[r]) != L.MSG_REPLY:
            out[r] = NOT_REPLY
        else:
            p = lead.get((0 if rec_conn is None else int(rec_conn[r]), int(xid[r])))
            if p is None:
                out[r] = UNKNOWN
            elif p in seen:
                out[r] = DUPLICATE
            else:
                seen.add(p)
                out[r] = p
                hit[p] = r
                tag[r] = pend["tag"][p]
    still = pend[hit == NONE].copy()
    result = np.array([int((out < FAILED).sum()), int((out == UNKNOWN).sum()), int((out == DUPLICATE).sum()),
                       int((out == NOT_REPLY).sum()), int((out == FAILED).sum()), len(still)], np.uint64)
    assert int(result[:5].sum()) == n
    return {"match": out, "hit": hit, "tag_out": tag, "still": still, "result": result}


def match_fast(msgs, status, rec_conn, pend):
    """match without its loops, for lists and batches of a million and more:
    the lead of a key is the first index np.unique finds for it in the list,
    the Replies look their keys up by np.searchsorted in the sorted distinct
    keys, and the first record that names a lead is again np.unique's first
    index. Sorting, where the kernels hash. Held against match in
    tests/test_match_model.py."""
    n, npend = len(msgs), len(pend)
    status = np.asarray(status, np.int32)
    out = np.where(status != 0, FAILED, NOT_REPLY).astype(np.uint32)
    hit = np.full(npend, NONE, np.uint32)
    tag = np.zeros(n, np.uint64)
    recs = np.flatnonzero((status == 0) & (msgs["msg_type"] == L.MSG_REPLY))
    conn = np.zeros(n, np.uint64) if rec_conn is None else np.asarray(rec_conn, np.uint64)
    rkey = (conn[recs] << np.uint64(32)) | msgs["xid"][recs].astype(np.uint64)
    pkey = (pend["conn"].astype(np.uint64) << np.uint64(32)) | pend["xid"].astype(np.uint64)
    distinct, lead = np.unique(pkey, return_index=True)
    at = np.minimum(np.searchsorted(distinct, rkey), max(len(distinct) - 1, 0))
    known = distinct[at] == rkey if len(distinct) else np.zeros(len(recs), bool)
    out[recs[~known]] = UNKNOWN
    p = lead[at[known]]                                # the lead each of these Replies names, in record order
    named, first = np.unique(p, return_index=True)
    out[recs[known]] = DUPLICATE
    winners = recs[known][first]
    out[winners] = named
    hit[named] = winners
    tag[winners] = pend["tag"][named]
    still = pend[hit == NONE].copy()
    result = np.array([int((out < FAILED).sum()), int((out == UNKNOWN).sum()), int((out == DUPLICATE).sum()),
                       int((out == NOT_REPLY).sum()), int((out == FAILED).sum()), len(still)], np.uint64)
    assert int(result[:5].sum()) == n
    return {"match": out, "hit": hit, "tag_out": tag, "still": still, "result": result}
