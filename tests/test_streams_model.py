"""The host model of segmented framing (tests/streams_model.py) against the
oracle's expected_message_len loop run once per segment, and the property
each slab builder was written for. No GPU."""
import numpy as np
import pytest

import frame_model as FM
import streams_model as SM


def _both(slab, off, ln, cap=None):
    m = SM.frame_streams(slab, off, ln, cap)
    o = SM.frame_streams_oracle(slab, off, ln, cap)
    assert m.same(o), "model != per-segment oracle"
    return m


@pytest.mark.parametrize("nseg", [1, 63, 64, 65, 129, 257])
def test_small_segments(nseg):
    slab, off, ln = SM.small_segments(nseg)
    m = _both(slab, off, ln)
    assert len(m.rows) == nseg and (m.rows[:, 3] == SM.OK).all()
    assert (m.rows[:, 1] <= 3).all() and int(m.rows[:, 1].sum()) == int(m.result[0]) == int(m.result[1])
    assert (m.rows[:, 2] == ln).all()                       # every segment consumed whole
    if nseg >= 63:
        assert set(m.rows[:, 1].tolist()) == {0, 1, 2, 3}
        assert len(set((off % 16).tolist())) > 8            # odd alignments
    # records ordered by segment, then by position
    assert (np.diff(m.rec_seg.astype(np.int64)) >= 0).all()
    assert np.array_equal(m.rows[:, 0], np.concatenate([[0], np.cumsum(m.rows[:-1, 1])]))


def test_reply_segments_cross_65536():
    slab, off, ln = SM.reply_segments()
    assert len(off) == 66_000 > 65_536
    m = SM.frame_streams(slab, off, ln)
    assert np.array_equal(m.rows[:, 1] * 28, ln) and set(m.rows[:, 1].tolist()) == {0, 1, 2}
    assert (m.rows[:, 3] == 0).all() and (m.rec_len == 28).all()
    sub = slice(65_500, 65_600)                             # the oracle on the stretch across 65536
    o = SM.frame_streams_oracle(slab, off[sub], ln[sub])
    lo = int(m.rows[65_500, 0])
    assert np.array_equal(o.rec_start, m.rec_start[lo:lo + len(o.rec_start)])


def test_stop_cases_between_healthy_neighbours():
    slab, off, ln, where = SM.stops_slab()
    m = _both(slab, off, ln)
    cases = SM.stop_cases()
    assert set(where) == set(cases) and len(off) == 2 * len(cases) + 1
    for name, s in where.items():
        assert tuple(int(x) for x in m.rows[s, 1:]) == cases[name][1], name
        for nb in (s - 1, s + 1):                           # three whole records each side
            assert tuple(int(x) for x in m.rows[nb, 1:]) == (3, int(ln[nb]), SM.OK, 0, 0), (name, nb)
    assert tuple(int(x) for x in m.rows[where["all ones"], 3:]) == (SM.INCOMPLETE_MESSAGE, 8, 0x80000003)
    st = m.rows[[where[k] for k in cases], 3].tolist()
    assert st == [0, 2, 2, 2, 1, 3, 3, 1]
    assert int(m.result[2]) == 7                            # the empty segment is OK


def test_marks_slab():
    slab, off, ln = SM.marks_slab()
    m = _both(slab, off, ln)
    assert m.rows[0::2, 1].tolist() == list(SM.MARK_COUNTS) and {64, 65, 200, SM.KEEP, SM.KEEP + 1} <= set(SM.MARK_COUNTS)
    assert (m.rows[1::2, 1] == 3).all() and (m.rows[:, 3] == 0).all()
    assert (m.rec_len[m.rec_seg % 2 == 0] == 4).all()


def test_long_slab():
    slab, off, ln = SM.long_slab()
    m = _both(slab, off, ln)
    assert int(ln[1]) == 1 << 20 and int(m.rows[1, 1]) > 5000
    assert int(m.rows[1, 3]) == SM.INCOMPLETE_MESSAGE and 0 < (1 << 20) - int(m.rows[1, 2]) == int(m.rows[1, 4]) < 300
    lens = m.rec_len[m.rec_seg == 1]
    assert lens.min() >= 28 and lens.max() <= 300
    assert m.rows[[0, 2], 1].tolist() == [3, 3]


def test_aligned_slab():
    slab, off, ln = SM.aligned_slab()
    m = _both(slab, off, ln)
    assert (off % 16).tolist() == list(range(16))
    assert (m.rows[:, 1] == 4).all() and (m.rows[:, 3] == 0).all()


def test_orders_and_repeats():
    slab, off, ln = SM.small_segments(65)
    a = _both(slab, off, ln)
    d = _both(slab, off[::-1], ln[::-1])                    # descending address order
    assert np.array_equal(d.rows[:, 1:], a.rows[::-1, 1:]) and (np.diff(d.rec_seg.astype(np.int64)) >= 0).all()
    t = _both(slab, np.concatenate([off, off]), np.concatenate([ln, ln]))
    n = int(a.result[0])
    assert int(t.result[0]) == 2 * n and np.array_equal(t.rec_start[:n], t.rec_start[n:])
    assert np.array_equal(t.rec_seg[n:], a.rec_seg + 65)


def capacity_values(slab, off, ln):
    full = SM.frame_streams(slab, off, ln)
    needed = int(full.result[1])
    f17, f18 = int(full.rows[17, 0]), int(full.rows[18, 0])
    return full, [0, 1, f17, f18, f17 + 40, needed - 1, needed, needed + 5]


def test_capacity_slab():
    slab, off, ln = SM.capacity_slab()
    full, caps = capacity_values(slab, off, ln)
    needed = int(full.result[1])
    assert len(off) == 40 and int(full.rows[17, 1]) == 65 and int(full.rows[30, 1]) == 100
    assert (full.rows[:, 3] != 0).sum() >= 3
    for cap in caps:
        m = _both(slab, off, ln, cap)
        assert int(m.result[1]) == (needed if cap else 0), cap
        assert int(m.result[0]) == min(cap, needed)
        if 0 < cap < needed:
            s = int(np.nonzero(m.rows[:, 0] + m.rows[:, 1] == cap)[0][0])   # the segment that reached it
            assert int(m.rows[s, 3]) == SM.OK
            later = m.rows[s + 1:]
            assert (later == np.array([cap, 0, 0, 0, 0, 0], np.uint64)).all()
            k = cap - int(full.rows[s, 0])
            if k < int(full.rows[s, 1]):                    # consumed = the first unframed record's start
                assert int(m.rows[s, 2]) == int(full.rec_start[cap]) - int(off[s])
        if cap == 0:
            assert not m.rows.any()
    m = SM.frame_streams(slab, off, ln, caps[4])
    assert int(m.rows[17, 1]) == 40                         # inside the 65-record segment


def test_connection_slab():
    slab, off, ln = SM.connection_slab()
    m = _both(slab, off, ln)
    assert len(off) == 100 and (off == np.arange(100) * SM.SLOT).all() and (ln <= SM.SLOT).all()
    st = m.rows[:, 3]
    assert int(st[37]) == SM.FRAGMENTED and int(m.rows[37, 1]) == 2
    assert tuple(int(x) for x in m.rows[61, 1:]) == (0, 0, 0, 0, 0) and int(ln[61]) == 0
    assert (st == SM.INCOMPLETE_MESSAGE).sum() + (st == SM.INCOMPLETE_HEADER).sum() > 50
    assert (st == SM.OK).sum() >= 20 and int(m.result[0]) > 500
    assert (m.rows[:, 2] <= ln).all()


def test_nseg_one_is_frame_stream():
    for buf in (FM.edge_stream(), FM.cut_stream(), FM.cut_stream()[:-7]):
        m = _both(buf, [0], [len(buf)])
        starts, stop, st, a0, a1 = FM.true_starts(buf)
        assert np.array_equal(m.rec_start.astype(np.int64), starts)
        assert tuple(int(x) for x in m.rows[0]) == (0, len(starts), stop, st, a0, a1)
