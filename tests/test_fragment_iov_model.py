"""The host model of onc_fragment_iov (tests/fragment_iov_model.py) against
the model of the packed path (fragment_encode_model.fragment), and the
property every built entry list claims: the GPU tests
(tests/test_gpu_fragment_iov.py) rely on both."""
import numpy as np
import pytest

import fragment_encode_model as E
import fragment_iov_model as V


def _same_as_packed(stream, F):
    iov, hdr, pay, wire, off = stream
    m = V.fragment_iov(iov, F)
    p = E.fragment(wire, off, F)
    assert V.gather(m["pieces"], m["marks"], hdr, pay) == E.stream_bytes(p)
    assert np.array_equal(m["out_off"], p["out_off"]) and np.array_equal(m["status"], p["status"])
    assert m["result"][:3].tolist() == p["result"].tolist()
    assert len(m["pieces"]) == int(m["result"][3]) == int(m["piece_off"][-1])
    assert len(m["marks"]) == 4 * int(m["result"][0])
    assert (m["pieces"]["len"] > 0).all()
    return m


def test_layouts_match_the_binding():
    import onc_rpc_amd.layout as L
    assert V.IOV_DTYPE == L.IOV_DTYPE and V.PIECE_DTYPE == L.FRAG_PIECE_DTYPE
    assert (V.PIECE_MARK, V.PIECE_HDR, V.PIECE_PAYLOAD) == (L.PIECE_MARK, L.PIECE_HDR, L.PIECE_PAYLOAD)
    assert E.MAX_FRAG_LIMIT == V.MAX_FRAG_LIMIT and (E.OK, E.ENC_WRITE_ZERO) == (V.OK, V.ENC_WRITE_ZERO)


@pytest.mark.parametrize("seed", range(6))
def test_random_splits_equal_the_packed_model(seed):
    stream = V.build(V.random_splits(80, seed), seed=seed)
    for F in (1, 2, 3, 7, 16, 59, 60, 61, 200, V.MAX_FRAG_LIMIT):
        m = _same_as_packed(stream, F)
        if F == V.MAX_FRAG_LIMIT:
            assert V.gather(m["pieces"], m["marks"], stream[1], stream[2]) == stream[3]


def test_invalid_entries_take_nothing():
    iov, hdr, pay, _, _ = V.build([(8, 2), (0, 5), (3, 0), (1, 9), (0, 0), (12, 0)])
    m = V.fragment_iov(iov, 4)
    assert m["status"].tolist() == [V.OK, V.ENC_BAD_DESCRIPTOR, V.ENC_BAD_DESCRIPTOR, V.ENC_BAD_DESCRIPTOR, V.OK, V.OK]
    assert np.diff(m["piece_off"].astype(np.int64)).tolist() == [4, 0, 0, 0, 0, 4]
    assert np.diff(m["out_off"].astype(np.int64)).tolist() == [6 + 8, 0, 0, 0, 0, 8 + 8]
    # the same records without the invalid entries: the same stream
    iov2 = iov[[0, 4, 5]]
    m2 = V.fragment_iov(iov2, 4)
    assert V.gather(m2["pieces"], m2["marks"], hdr, pay) == V.gather(m["pieces"], m["marks"], hdr, pay)


def test_capacity_cut_is_a_prefix():
    iov, hdr, pay, _, _ = V.build(V.random_splits(40, 9), seed=9)
    full = V.fragment_iov(iov, 16)
    tot_p, tot_m = int(full["result"][3]), 4 * int(full["result"][0])
    for kw in ({"max_pieces": 0}, {"max_pieces": tot_p - 1}, {"max_pieces": tot_p // 2}, {"marks_cap": 0},
               {"marks_cap": tot_m - 1}, {"marks_cap": tot_m // 2 + 1}, {"marks_cap": 7, "max_pieces": tot_p}):
        m = V.fragment_iov(iov, 16, **kw)
        for k in ("out_off", "piece_off", "result"):
            assert np.array_equal(m[k], full[k])
        w = len(m["pieces"])
        assert np.array_equal(m["pieces"], full["pieces"][:w]) and m["marks"] == full["marks"][:len(m["marks"])]
        st = m["status"].tolist()
        first = st.index(V.ENC_WRITE_ZERO)
        assert w == int(full["piece_off"][first]) and w <= kw.get("max_pieces", w)
        assert len(m["marks"]) <= kw.get("marks_cap", len(m["marks"]))
        takes = np.diff(full["piece_off"].astype(np.int64)) > 0
        assert all(s == V.ENC_WRITE_ZERO for s, t in zip(st[first:], takes[first:]) if t)


@pytest.mark.parametrize("F", V.BOUNDARY_FS)
def test_boundary_stream(F):
    iov, hdr, pay, wire, off = V.boundary_stream(F)
    hl, pl = iov["hdr_len"].astype(np.int64), iov["payload_len"].astype(np.int64)
    assert hl[0] + pl[0] == 0 and hl[-1] + pl[-1] == 0
    empty = (hl + pl) == 0
    assert (empty[1:] & empty[:-1]).any()
    assert ((hl == 0) & (pl > 0)).sum() == 1
    assert {1, 3, 4, 5, 4 + F - 1, 4 + F, 4 + F + 1, 4 + 2 * F} <= set(hl.tolist())
    for h in (4, 5, 4 + F - 1, 4 + F, 4 + F + 1, 4 + 2 * F):
        assert {0, 1, F - 1, F, F + 1, 2 * F + 1} <= set(pl[hl == h].tolist())
    m = V.fragment_iov(iov, F)
    assert set(m["status"].tolist()) == {V.OK, V.ENC_BAD_DESCRIPTOR}
    # the valid entries alone are the packed stream's records
    ok = (hl >= 4) | empty
    keep = np.nonzero(ok)[0]
    w = b"".join(wire[int(off[i]):int(off[i + 1])] for i in keep)
    o = np.concatenate(([0], np.cumsum((hl + pl)[keep]))).astype(np.uint64)
    assert V.gather(m["pieces"], m["marks"], hdr, pay) == E.stream_bytes(E.fragment(w, o, F))


@pytest.mark.parametrize("t", sorted(V.STRADDLE_KINDS))
def test_tile_straddle_stream(t):
    stream = V.tile_straddle_stream(t)
    m = _same_as_packed(stream, V.STRADDLE_F)
    rec = V.TILE - t
    assert int(m["piece_off"][rec]) == V.TILE - t and int(m["piece_off"][rec + 1]) == V.TILE - t + 7
    assert int(m["pieces"]["src"][V.TILE]) == V.STRADDLE_KINDS[t]
    assert m["pieces"]["src"][V.TILE - t:V.TILE - t + 7].tolist() == [0, 1, 0, 1, 2, 0, 2]
    assert set(V.STRADDLE_KINDS.values()) == {V.PIECE_MARK, V.PIECE_HDR, V.PIECE_PAYLOAD}


def test_bare_marks_stream():
    m = _same_as_packed(V.bare_marks_stream(), 16)
    assert V.records_reaching_into_tiles(m).max() > V.STAGE
    iov = V.bare_marks_stream()[0]
    assert ((iov["hdr_len"] == 0) & (iov["payload_len"] == 0)).sum() >= 1000
    assert ((iov["hdr_len"] == 4) & (iov["payload_len"] == 0)).sum() >= 3000


def test_large_record_stream():
    m = _same_as_packed(V.large_record_stream(), 7)
    assert int(np.diff(m["piece_off"].astype(np.int64)).max()) > 4 * V.TILE


@pytest.mark.parametrize("n", [255, 256, 257, 1025])
def test_short_records(n):
    stream = V.short_records(n)
    L = stream[0]["hdr_len"].astype(np.int64) + stream[0]["payload_len"]
    assert len(L) == n and L.min() >= 4 and L.max() <= 40
    _same_as_packed(stream, 9)


def test_per_record_stream():
    (iov, hdr, pay, wire, off), lim = V.per_record_stream()
    assert set(V.PER_RECORD_LIMITS) == set(lim.tolist())
    bad = (lim < 1) | (lim > V.MAX_FRAG_LIMIT)
    assert not (bad[1:] & bad[:-1]).any() and not bad[0] and not bad[-1]
    m = V.fragment_iov(iov, 16, rec_max_frag=lim)
    L = iov["hdr_len"].astype(np.int64) + iov["payload_len"]
    assert (m["status"][bad & (L > 0)] == V.ENC_BAD_DESCRIPTOR).all() and (m["status"][~bad] == V.OK).all()
    assert (bad & (L > 0)).sum() >= 3
    # each valid record is what the uniform call at its own limit makes of it
    at, mk = 0, 0
    for i in range(len(iov)):
        if bad[i] or L[i] == 0:
            continue
        one = V.fragment_iov(iov[i:i + 1], int(lim[i]))
        e = len(one["pieces"])
        got = m["pieces"][at:at + e].copy()
        is_mark = got["src"] == V.PIECE_MARK
        got["off"][is_mark] -= mk
        assert np.array_equal(got, one["pieces"]) and m["marks"][mk:mk + len(one["marks"])] == one["marks"]
        at += e
        mk += len(one["marks"])
    assert at == len(m["pieces"]) and mk == len(m["marks"])
    # an array filled with one value is the uniform call
    u = V.fragment_iov(iov, 16, rec_max_frag=np.full(len(iov), 16, np.uint32))
    v = V.fragment_iov(iov, 16)
    assert all(np.array_equal(u[k], v[k]) for k in ("pieces", "out_off", "piece_off", "status", "result"))
    assert u["marks"] == v["marks"]
