"""The plan and partition scans past their first round. Six calls reduce
per-block or per-tile counts in one workgroup that walks them in rounds and
carries a running aggregate from a round to the next (the table in
tests/scan_rounds_cases.py): every other test of the suite stays inside the
first round, where the carry is the identity and the loop body runs once.
Here every count reaches the second round and the third, and every output
array is compared whole and bit-exactly with the call's host model, the
sentinels behind and around it included, as in the sibling files whose
checks these cases go through.

  call                a second round          a third round
  onc_fragment_iov    n = 65537, 65793        n = 131073
  onc_piece_offsets   npieces = 65537, 65793  npieces = 131073
  onc_payload_slots   n = 65537, 65793        n = 131073
  onc_route_calls     n = 262145, 263169      n = 524289
  onc_group_by_conn   n = 262145              n = 524289   (every radix pass)
  onc_match_replies   np = 1048577            np = 2097153 (the unanswered counts)
                      n = 1049576: the class sums' second stride

The round lengths are pinned by a static_assert next to kCopyThreads,
kRtScanThreads, kGrFlat and kMtThreads. The same sizes are the first above
the floor of the scratch (65536 elements): the first case of each call runs
on a fresh handle, which allocates it above the floor, the others on one
handle that has made a small call, which regrows a used one.
tests/test_scan_rounds_model.py proves on the CPU, from the same inputs, that
a scan without its carry fails each of these comparisons."""
import contextlib

import numpy as np
import pytest

import fragment_iov_model as V
import group_model as GM
import match_model as MM
import payload_model as PM
import route_model as RM
import scan_rounds_cases as C
from test_gpu_fragment_iov import _fiv
from test_gpu_gather import Listed
from test_gpu_group import _check as _group_check
from test_gpu_match import _compare as _match_compare

pytestmark = pytest.mark.gpu

SENT = C.SENT
U32, U64 = 0xFFFFFFFF, np.uint64(2**64 - 1)


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def used(R):
    """One handle for the module that has made a small call: its scratch is
    there, at the floor, before the first case regrows it."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = R.Codec(0)
    g = R.group_by_conn_host(c, np.arange(10, dtype=np.uint32) % 3, None, 3)
    assert g["result"].tolist() == [10, 0, 3]
    yield c
    c.close()


@contextlib.contextmanager
def _handle(R, used, fresh):
    """A handle of its own, whose scratch the case allocates, or the module's."""
    if not fresh:
        yield used
        return
    c = R.Codec(0)
    try:
        yield c
    finally:
        c.close()


# ---------------------------------------------------------------------------
# onc_fragment_iov: fragiov_blkscan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.PLAN_SIZES)
def test_fragment_iov(R, used, n):
    """marks, pieces, out_off, piece_off, status and result against the model
    (test_gpu_fragment_iov._fiv). R + 1: a second round of one block holding
    one record; R + 257: a partial third block of round two; 2 R + 1: a third
    round."""
    iov, _ = C.fiv_case(n)
    with _handle(R, used, fresh=n == C.PLAN_SIZES[0]) as c:
        m = _fiv(R, c, iov, C.FIV_F)
    assert int(m["result"][2]) > n // 2                                # most records split
    assert {V.OK, V.ENC_BAD_DESCRIPTOR} == set(m["status"].tolist())


def test_fragment_iov_with_a_limit_per_record(R, used):
    n = C.R_PLAN + 257
    iov, lim = C.fiv_case(n, per_record=True)
    m = _fiv(R, used, iov, C.FIV_F, lim=lim)
    bad = (lim < 1) | (lim > 0x7FFFFFFF)
    assert bad[:C.R_PLAN].any() and bad[C.R_PLAN:].any()
    assert (m["status"][bad & (iov["hdr_len"] >= 4)] == V.ENC_BAD_DESCRIPTOR).all()

# ---------------------------------------------------------------------------
# onc_piece_offsets: gath_blkscan; then onc_gather_pieces of the whole stream
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,bad", C.GATHER_CASES)
def test_piece_offsets_and_gather(R, used, n, bad):
    """piece_pos and result against the model (test_gpu_gather.Listed), then
    the whole stream gathered at two alignments. "late": the carry holds no bad
    piece when the first one comes; "both": first_bad stays the early one and
    `bad` counts them all. (A first bad piece in round two with more behind it
    takes three pieces there, bad pieces in two rounds take two rounds: the
    sizes that have neither run without.)"""
    pieces, sources, where = C.gather_case(n, bad)
    with _handle(R, used, fresh=(n, bad) == C.GATHER_CASES[0]) as c:
        lst = Listed(R, c, pieces, sources)
        assert lst.res.tolist()[1:] == [len(where), where[0] if where else n]
        if bad == "late":
            assert where[0] >= C.R_PLAN
        if bad == "both":
            assert where[0] < C.R_PLAN <= where[-1]
        for shift in (0, 5):
            lst.window(0, lst.total, shift)


# ---------------------------------------------------------------------------
# onc_payload_slots: pay_blkscan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("align", [16, 4096])
@pytest.mark.parametrize("n", C.PLAN_SIZES)
def test_payload_slots(R, used, n, align):
    """pay_pos, pay_len, slot_off (slot_off[n] included), result and msgs_out
    against the model, with and without msgs_out; the comparisons of
    test_gpu_payload._check_slots with the model worked out once."""
    m, status = C.payload_case(n)
    want = PM.payload_slots(m, status, align, head_len=C.PAY_HEAD, want_msgs_out=True)
    assert set(want["pay_len"].tolist()) == set(C.PAY_LENS) and int(want["result"][0]) > n // 3
    src = m.view(np.uint8).reshape(-1)
    with _handle(R, used, fresh=(n, align) == (C.PLAN_SIZES[0], 16)) as c:
        for out_mode in (None, "separate"):
            g = R.payload_slots_host(c, m, status, align, head_len=C.PAY_HEAD, msgs_out=out_mode)
            raw, what = g["raw"], f"n {n} align {align} msgs_out {out_mode}"
            assert g["result"].tolist() == want["result"].tolist(), f"{what}: result {g['result']} != {want['result']}"
            assert (raw["result"][3:] == U64).all()
            for k in ("pay_pos", "pay_len"):
                assert np.array_equal(raw[k][:n], want[k]), f"{what}: {k}"
                assert (raw[k][n:] == U32).all(), f"{what}: {k} written past n"
            bad = np.flatnonzero(raw["slot_off"][:n + 1] != want["slot_off"])
            assert len(bad) == 0, (f"{what}: slot_off differs first at record {bad[0]} (round {bad[0] // C.R_PLAN}): "
                                   f"{raw['slot_off'][bad[0]]} != {want['slot_off'][bad[0]]}")
            assert (raw["slot_off"][n + 1:] == U64).all(), f"{what}: slot_off written past n + 1"
            assert np.array_equal(raw["msgs"][:64 * n], src), f"{what}: msgs changed"
            assert (raw["msgs"][64 * n:] == SENT).all()
            if out_mode == "separate":
                assert np.array_equal(raw["msgs_out"][:64 * n], want["msgs_out"].view(np.uint8).reshape(-1)), \
                    f"{what}: msgs_out"
                assert (raw["msgs_out"][64 * n:] == SENT).all()
            else:
                assert g["msgs_out"] is None


# ---------------------------------------------------------------------------
# onc_route_calls: route_scan_bins
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which,n,shape", C.ROUTE_CASES)
def test_route_calls(R, used, which, n, shape):
    """route, order, bin_first, result, calls_out and replies against the
    model; the comparisons of test_gpu_route._check for the call with both
    optional outputs. "every": every bin has records on both sides of tile 256;
    "late": one handler bin's records all lie at index >= R (its carry is 0,
    and the bins behind it depend on its total); "early": one bin's records all
    lie below R. (n = R has no record at or behind R: it runs "every" alone.)"""
    msgs, status, tab, nh, bins, B = C.route_case(n, which, shape)
    want = RM.route_calls_fast(msgs, status, tab, nh)
    assert np.array_equal(want["route"], bins)
    with _handle(R, used, fresh=(which, n, shape) == C.ROUTE_CASES[0]) as c:
        g = R.route_calls_host(c, msgs, status, tab, nh, calls_out=True, replies=True)
    raw, w = g["raw"], f"{which} table, n {n}, {shape}"
    assert g["result"].tolist() == want["result"].tolist(), f"{w}: result {g['result']} != {want['result']}"
    assert (raw["result"][4:] == U64).all(), f"{w}: result written past 4"
    assert np.array_equal(g["bin_first"], want["bin_first"]), f"{w}: bin_first"
    assert (raw["bin_first"][nh + 4:] == U64).all(), f"{w}: bin_first written past nh + 4"
    assert np.array_equal(g["route"], want["route"]), f"{w}: route"
    bad = np.flatnonzero(g["order"] != want["order"])
    assert len(bad) == 0, (f"{w}: order differs first at place {bad[0]}: record {g['order'][bad[0]]} (tile "
                           f"{g['order'][bad[0]] // C.TILE}) != {want['order'][bad[0]]}; {len(bad)} places differ")
    for k in ("route", "order"):
        assert (raw[k][n:] == U32).all(), f"{w}: {k} written past n"
    for k in ("calls_out", "replies"):
        assert g[k].tobytes() == want[k].tobytes(), f"{w}: {k}"
        assert (raw[k][64 * n:] == SENT).all(), f"{w}: {k} written past n"
    # stability, directly: order is strictly increasing inside each bin, and a permutation
    o, first = g["order"].astype(np.int64), g["bin_first"].astype(np.int64)
    inside = np.ones(n, bool)
    inside[first[(first > 0) & (first < n)]] = False
    assert (np.diff(o)[inside[1:]] > 0).all(), f"{w}: order not ascending inside a bin"
    assert np.array_equal(np.sort(o), np.arange(n)), f"{w}: order is no permutation"


# ---------------------------------------------------------------------------
# onc_group_by_conn: group_scan_digits, once per radix pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,nconn,with_via", C.GROUP_CASES)
def test_group_by_conn(R, used, n, nconn, with_via):
    """order, conn_first, result and msgs_out against the model, and the
    direct stability and permutation assertions (test_gpu_group._check). 200
    connections: one pass; 70 000: three, the later ones reading the (key,
    index) pairs the pass before left in the scratch above its floor."""
    assert GM.passes(nconn) == {200: 1, 70000: 3}[nconn]
    rec_conn, via = C.group_case(n, nconn, with_via)
    with _handle(R, used, fresh=(n, nconn, with_via) == C.GROUP_CASES[0]) as c:
        want = _group_check(R, c, rec_conn, via, nconn, "scan rounds", with_msgs=(True,))
    assert int(want["result"][1]) > n // 50 and int(want["result"][2]) > 150       # dropped items; many groups


# ---------------------------------------------------------------------------
# onc_match_replies: match_scan
# ---------------------------------------------------------------------------
def _match(R, c, case, outputs, what):
    msgs, status, rec_conn, pend = case
    want = MM.match_fast(msgs, status, rec_conn, pend)
    g = R.match_replies_host(c, msgs, status, rec_conn, pend, tag_out=outputs, still=outputs)
    _match_compare(g, want, len(msgs), len(pend), outputs, outputs, what)
    return want


@pytest.mark.parametrize("npend,answer_last,outputs", C.MATCH_PENDING)
def test_match_replies_pending_side(R, used, npend, answer_last, outputs):
    """match, hit, tag_out, still and result against the model
    (test_gpu_match._compare), 3073 records against a list that takes the
    scan of the unanswered counts into its second and third round. Most
    entries stay unanswered in every round, so `still` and result[5] depend on
    the carry. The last entry is a round's only one: left unanswered its place
    in `still` is the carry itself; answered, the Reply hits the last round's
    tile. The first case again without tag_out and still."""
    *case, answered = C.match_pending_case(npend, answer_last)
    with _handle(R, used, fresh=(npend, answer_last, outputs) == C.MATCH_PENDING[0]) as c:
        want = _match(R, c, case, outputs, f"np {npend}, last entry answered {answer_last}, outputs {outputs}")
    assert np.array_equal(np.flatnonzero(want["hit"] != MM.NONE), answered)
    assert int(want["result"][5]) == npend - len(answered) and (want["result"][:5] > 0).all()
    assert (answered < 3 * C.TILE).sum() == 1500 and (answered[-1] == npend - 1) == answer_last
    if npend > 2 * C.R_MATCH:
        assert ((answered >= C.R_MATCH) & (answered < 2 * C.R_MATCH)).sum() == 900


def test_match_replies_record_side(R, used):
    """R + 1000 records against 5000 entries: every class sum takes its second
    stride over the record tiles, and each class has records on both sides of
    record R."""
    case = C.match_record_case()
    want = _match(R, used, case, True, "record side")
    m = want["match"]
    for part in (m[:C.R_MATCH], m[C.R_MATCH:]):
        assert (part < MM.FAILED).any()
        assert all((part == v).any() for v in (MM.UNKNOWN, MM.DUPLICATE, MM.NOT_REPLY, MM.FAILED))
