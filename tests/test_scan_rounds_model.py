"""The proof, on the CPU, that the cases of tests/test_gpu_scan_rounds.py
bite: from the host model's right result for the very inputs the GPU file
runs (tests/scan_rounds_cases.py builds them for both), what the call would
have written had its one-workgroup scan dropped the carry between rounds is
constructed — every element a round k > 0 owns short of the totals of the
rounds before k, the batch totals the last round's alone — and shown to
differ from the right result in every output that the scan feeds. (What a
call works out per element from its input alone — status, pay_pos and
pay_len, route, match, hit and tag_out — no scan can change; the test says so
by leaving them out, and the GPU file compares them all the same.) A count of
exactly one round is the control: there the construction must change nothing.
The shapes built for a purpose are checked for it. No GPU."""
import numpy as np
import pytest

import fragment_iov_model as V
import gather_model as G
import group_model as GM
import match_model as MM
import payload_model as PM
import route_model as RM
import scan_rounds_cases as C


def _differs(right, wrong, keys, n, R, what):
    """Every named output differs when the scan takes more than one round, and
    none when it takes one."""
    for k in keys:
        a, b = np.asarray(right[k]), np.asarray(wrong[k])
        same = a.tobytes() == b.tobytes()
        if C.rounds(n, R) > 1:
            assert not same, f"{what}: a scan without its carry would write the right {k}"
        else:
            assert same, f"{what}: one round, and the construction changes {k}"


def test_round_lengths():
    """The numbers of the static_asserts in tile_walk.h, route.hip, group.hip
    and match.hip, and what the cases make of them."""
    assert (C.R_PLAN, C.R_ROUTE, C.R_GROUP, C.R_MATCH) == (65536, 262144, 262144, 1048576)
    assert [C.rounds(n, C.R_PLAN) for n in C.PLAN_SIZES] == [1, 2, 2, 3]
    assert [C.rounds(n, C.R_ROUTE) for n in C.ROUTE_SIZES] == [1, 2, 2, 3]
    assert [C.rounds(n, C.R_GROUP) for n in C.GROUP_SIZES] == [2, 3]
    assert sorted({C.rounds(-(-np_ // C.TILE), C.TILE) for np_, _, _ in C.MATCH_PENDING}) == [2, 3]
    assert C.rounds(-(-C.MATCH_REC_N // C.TILE), C.TILE) == 2
    # R + 257: round two holds two whole blocks of 256 and one record of a third
    assert (C.PLAN_SIZES[2] - C.R_PLAN) // 256 == 1 and (C.PLAN_SIZES[2] - C.R_PLAN) % 256 == 1


def test_drop_carry():
    p = np.array([0, 1, 3, 6, 10, 15, 21])                            # the prefix of 1 .. 6
    assert C.drop_carry(p, 6).tolist() == p.tolist() and C.drop_carry(p, 7).tolist() == p.tolist()
    assert C.drop_carry(p, 2).tolist() == [0, 1, 0, 3, 0, 5, 11]       # rounds (1 2) (3 4) (5 6); the last one's total
    assert C.drop_carry(p, 4).tolist() == [0, 1, 3, 6, 0, 5, 11]
    assert C.drop_carry(p, 5).tolist() == [0, 1, 3, 6, 10, 0, 6]       # a last round of one element
    dest, first = C.partition_without_carry([1, 0, 1, 1, 0, 1], 2, 4)  # rounds (1 0 1 1) (0 1): totals 1 and 1
    assert first.tolist() == [0, 1, 2] and dest.tolist() == [1, 0, 2, 3, 0, 1]
    dest, first = C.partition_without_carry([1, 0, 1, 1, 0, 1], 2, 6)  # one round: the stable partition
    assert first.tolist() == [0, 2, 6] and dest.tolist() == [2, 0, 3, 4, 1, 5]


# ---------------------------------------------------------------------------
# the three plan scans
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,per_record", [(n, False) for n in C.PLAN_SIZES] + [(C.R_PLAN + 257, True)])
def test_fragment_iov_cases(n, per_record):
    iov, lim = C.fiv_case(n, per_record)
    m = V.fragment_iov(iov, C.FIV_F, lim)
    right = dict(m, pieces=m["pieces"].view(np.uint8), marks=np.frombuffer(m["marks"], np.uint8))
    _differs(right, C.fiv_lost_carry(m), ("out_off", "piece_off", "result", "pieces", "marks"), n, C.R_PLAN,
             f"onc_fragment_iov n {n}")
    # failing records and placeholders on both sides of record R, which itself takes pieces
    st, took = m["status"], np.diff(m["piece_off"].astype(np.int64)) > 0
    empty = (iov["hdr_len"] == 0) & (iov["payload_len"] == 0)
    for part in (slice(0, C.R_PLAN),) + ((slice(C.R_PLAN, n),) if n >= C.R_PLAN + 3 else ()):
        assert (st[part] == V.ENC_BAD_DESCRIPTOR).any() and empty[part].any()
    assert took[C.R_PLAN - 1] and (n == C.R_PLAN or took[C.R_PLAN])


@pytest.mark.parametrize("n,bad", C.GATHER_CASES)
def test_gather_cases(n, bad):
    pieces, sources, where = C.gather_case(n, bad)
    lens = list(C.GATHER_LENS)
    pos, res = G.piece_offsets(pieces, lens)
    assert [i for i, (o, ln, s) in enumerate(pieces.tolist()) if not G.ok(o, ln, s, lens)] == where
    assert set(pieces["len"].tolist()) == {0, 1, 2, 3} and set(pieces["src"][pieces["src"] < 3].tolist()) == {0, 1, 2}
    stream = G.gather(pieces, pos, sources, 0, int(res[0]), np.full(int(res[0]), C.SENT, np.uint8))
    w_pos, w_res, w_stream = C.gather_lost_carry(pieces, sources, pos, res, where)
    # (R + 1 pieces with a bad one in both rounds: round two's only piece is the bad one, which writes nothing — there
    # the positions and the result depend on the carry and the bytes cannot)
    keys = ("piece_pos", "result") if (n, bad) == (C.R_PLAN + 1, "both") else ("piece_pos", "result", "stream")
    _differs({"piece_pos": pos, "result": res, "stream": stream},
             {"piece_pos": w_pos, "result": w_res, "stream": w_stream}, keys, n, C.R_PLAN,
             f"onc_piece_offsets n {n} bad {bad}")
    if bad == "late":
        # the carry holds no bad piece when the first one comes, and more follow it
        assert where[0] >= C.R_PLAN and len(where) >= 3 and res.tolist()[1:] == [len(where), where[0]]
    if bad == "both":
        # first_bad is the early one, the last round alone would name a later one and count fewer
        assert where[0] < C.R_PLAN <= where[-1] and res.tolist()[1:] == [len(where), where[0]]
        assert int(w_res[2]) > where[0] and int(w_res[1]) < len(where)


@pytest.mark.parametrize("align", [16, 4096])
@pytest.mark.parametrize("n", C.PLAN_SIZES)
def test_payload_cases(n, align):
    m, status = C.payload_case(n)
    want = PM.payload_slots(m, status, align, head_len=C.PAY_HEAD, want_msgs_out=True)
    _differs(want, C.payload_lost_carry(want), ("slot_off", "result", "msgs_out"), n, C.R_PLAN,
             f"onc_payload_slots n {n} align {align}")
    assert set(want["pay_len"].tolist()) == set(C.PAY_LENS) and (status != 0).any()
    if n > C.R_PLAN:
        assert want["pay_len"][C.R_PLAN] > 0                           # round two's first record takes a slot


# ---------------------------------------------------------------------------
# the two partitions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which,n,shape", C.ROUTE_CASES)
def test_route_cases(which, n, shape):
    msgs, status, tab, nh, bins, B = C.route_case(n, which, shape)
    assert RM.first_bad(tab, nh) == 0 and (which == "small" or (len(tab), nh + 3) == (1024, 256))
    want = RM.route_calls_fast(msgs, status, tab, nh)
    assert np.array_equal(want["route"], bins)
    right = dict(want, calls_out=want["calls_out"].view(np.uint8), replies=want["replies"].view(np.uint8))
    _differs(right, C.route_lost_carry(msgs, want, nh), ("order", "bin_first", "result", "calls_out", "replies"), n,
             C.R_ROUTE, f"onc_route_calls {which} n {n} {shape}")
    # served, rejected in all three ways, no Call, failed
    stats = {RM.ACCEPT_SUCCESS, RM.PROG_UNAVAIL, RM.PROG_MISMATCH, RM.PROC_UNAVAIL}
    assert stats <= set(want["stat"][bins <= nh].tolist())
    assert (want["result"][:3] > 0).all()
    R, first = C.R_ROUTE, want["bin_first"].astype(np.int64)
    early, late = np.bincount(bins[:R], minlength=nh + 3), np.bincount(bins[R:], minlength=nh + 3)
    if shape == "every":
        assert (early > 0).all() and (late > 0).sum() == min(nh + 3, n - R)
    elif shape == "late":
        # the bin's carry is 0, its total is not, and the bins behind it start after it
        assert early[B] == 0 and late[B] >= 1 and first[B + 1] - first[B] == late[B]
        assert (late[B + 1:] + early[B + 1:] > 0).all()
    else:
        assert late[B] == 0 and early[B] >= 1 and first[B + 1] - first[B] == early[B]


@pytest.mark.parametrize("n,nconn,with_via", C.GROUP_CASES)
def test_group_cases(n, nconn, with_via):
    rec_conn, via = C.group_case(n, nconn, with_via)
    msgs = C.descriptors(n, seed=n)                                    # (what test_gpu_group._check gathers)
    want = GM.group(rec_conn, via, nconn, msgs=msgs)
    key = GM.keys(rec_conn, via, nconn)
    _differs(want, C.group_lost_carry(key, nconn, msgs), ("order", "conn_first", "result", "msgs_out"), n, C.R_GROUP,
             f"onc_group_by_conn n {n} nconn {nconn}")
    assert len(key) == n and (key == nconn).sum() > n // 50
    if with_via:
        assert len(rec_conn) == n + 9 and len(set(via.tolist())) == n
    # every digit of every pass has items in every round: each pass's scan carries
    for p in range(GM.passes(nconn)):
        d = (key >> np.uint64(8 * p)) & np.uint64(255)
        for lo in range(0, n - 1, C.R_GROUP):                          # (the last round of one item aside)
            assert len(set(d[lo:lo + C.R_GROUP].tolist())) == len(set(d.tolist()))


# ---------------------------------------------------------------------------
# onc_match_replies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("npend,answer_last", sorted({(a, b) for a, b, _ in C.MATCH_PENDING}))
def test_match_pending_cases(npend, answer_last):
    msgs, status, rec_conn, pend, answered = C.match_pending_case(npend, answer_last)
    assert len(msgs) == C.MATCH_N and len(set(zip(pend["conn"].tolist(), pend["xid"].tolist()))) == npend
    want = MM.match_fast(msgs, status, rec_conn, pend)
    wrong = C.match_lost_carry(pend, want, len(msgs))
    k = len(want["still"])
    assert wrong["result"][:5].tolist() == want["result"][:5].tolist()           # three record tiles: one stride
    waiting = want["hit"] == MM.NONE
    assert int(wrong["result"][5]) != k
    # (R + 1 entries with the last one answered: no entry waits behind round one, so result[5] alone is the carry)
    assert (wrong["still"][:16 * k].tobytes() != want["still"].tobytes()) == bool(waiting[C.R_MATCH:].any())
    assert waiting[C.R_MATCH:].any() or (npend, answer_last) == (C.R_MATCH + 1, True)
    assert np.array_equal(np.flatnonzero(~waiting), answered) and (want["result"][:5] > 0).all()
    # most entries wait in every round; the last entry, a round's only one, as asked
    for lo in range(0, npend - 1, C.R_MATCH):
        assert waiting[lo:lo + C.R_MATCH].sum() > C.R_MATCH - 2000
    assert waiting[npend - 1] == (not answer_last)
    if not answer_last:
        # its place in `still` is the carry: without it the entry lands at 0
        assert want["still"][k - 1].tobytes() == pend[npend - 1].tobytes()
        assert wrong["still"][:16].tobytes() == pend[npend - 1].tobytes()


def test_match_record_case():
    msgs, status, rec_conn, pend = C.match_record_case()
    n = len(msgs)
    assert (n, len(pend)) == (C.R_MATCH + 1000, 5000)
    want = MM.match_fast(msgs, status, rec_conn, pend)
    wrong = C.match_lost_carry(pend, want, n)
    # every class sum is short without the first stride's tile 0, and every class has records there
    assert (wrong["result"][:5] < want["result"][:5]).all()
    m = want["match"]
    for part in (m[:C.TILE], m[:C.R_MATCH], m[C.R_MATCH:]):
        assert (part < MM.FAILED).any()
        assert all((part == v).any() for v in (MM.UNKNOWN, MM.DUPLICATE, MM.NOT_REPLY, MM.FAILED))
    assert 0 < len(want["still"]) < 5000
