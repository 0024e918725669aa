"""The host model of onc_frame_fragment_streams and onc_defragment_extents
(tests/fragment_streams_model.py) against the single-stream models it
generalises (fragment_model.frame_fragments + defragment run once per
segment), and the property each slab builder was written for. No GPU."""
import numpy as np
import pytest

import fragment_model as FR
import fragment_streams_model as FS
import streams_model as SM


def random_slab(seed):
    rng = np.random.default_rng(seed)
    sl = SM.Slab(front=int(rng.integers(0, 16)))
    for _ in range(int(rng.integers(1, 9))):
        data = b"".join(FS.record(rng, int(rng.integers(1, 8))) for _ in range(int(rng.integers(0, 5))))
        data += FS.ending(rng, FS.ENDINGS[int(rng.integers(0, 4))])[0]
        sl.add(data, gap=int(rng.integers(0, 12)))
    return sl.done()


def check_against_single_stream(slab, off, ln, m):
    """Per segment {n, consumed, n_rec, status, aux} are those of
    frame_fragments + defragment of the segment alone."""
    k = r = 0
    for s in range(len(off)):
        buf = slab[int(off[s]):int(off[s]) + int(ln[s])]
        fo, nf, _, st, a0, a1 = FR.frame_fragments(buf)
        d = FR.defragment(buf, fo)
        n_rec, consumed, pending = int(d["result"][0]), int(d["result"][1]), int(d["result"][3])
        want = (k, nf - pending, consumed, st, a0, a1, r, n_rec)
        assert tuple(int(x) for x in m.rows[s]) == want, (s, m.rows[s], want)
        lo, hi = k, k + nf - pending
        assert np.array_equal(m.frag_start[lo:hi], fo[:nf - pending] + np.uint64(off[s]))
        assert np.array_equal(m.frag_len[lo:hi].astype(np.int64), np.diff(fo.astype(np.int64))[:nf - pending])
        assert (m.frag_seg[lo:hi] == s).all()
        k, r = hi, r + n_rec
    assert m.result.tolist() == [k, k, r, int((m.rows[:, 3] != 0).sum())]


def check_capacities(slab, off, ln, full):
    needed = int(full.result[1])
    for cap in range(0, needed + 2):
        m = FS.frame_fragment_streams(slab, off, ln, cap)
        if cap == 0:
            assert not m.rows.any() and not m.result.any() and len(m.frag_start) == 0
            continue
        n = int(m.result[0])
        assert int(m.result[1]) == needed and n <= cap
        for k in ("frag_start", "frag_len", "frag_seg"):
            assert np.array_equal(getattr(m, k), getattr(full, k)[:n]), (cap, k)
        if cap >= needed:
            assert m.same(full), cap
            continue
        # whole records only: the emitted list ends with a last fragment
        assert n == 0 or slab[int(m.frag_start[-1])] & 0x80
        cut = int(np.nonzero(full.rows[:, 0] + full.rows[:, 1] > cap)[0][0])
        assert np.array_equal(m.rows[:cut], full.rows[:cut])
        assert int(m.rows[cut, 3]) == FS.OK and int(m.rows[cut, 0]) + int(m.rows[cut, 1]) == n
        assert int(m.rows[cut, 6]) + int(m.rows[cut, 7]) == int(m.result[2])
        assert (m.rows[cut + 1:] == np.array([cap, 0, 0, 0, 0, 0, 0, 0], np.uint64)).all()
        # the next record did not fit
        nxt = full.frag_seg[n:] == cut
        first_rec_frags = int(np.nonzero([slab[int(a)] & 0x80 for a in full.frag_start[n:]])[0][0]) + 1
        assert nxt[:first_rec_frags].all() and n + first_rec_frags > cap


@pytest.mark.parametrize("seed", range(40))
def test_random_slabs(seed):
    slab, off, ln = random_slab(1000 + seed)
    m = FS.frame_fragment_streams(slab, off, ln)
    check_against_single_stream(slab, off, ln, m)
    # the emitted extents, concatenated, defragment with nothing pending
    d = FS.defragment_extents(slab, m.frag_start, m.frag_len)
    assert d["result"].tolist()[:2] == [int(m.result[2]), int(m.result[0])] and not d["result"][3:5].any()
    check_capacities(slab, off, ln, m)


@pytest.mark.parametrize("nseg", [63, 64, 65, 129, 257])
def test_random_segments(nseg):
    slab, off, ln = FS.random_segments(nseg)
    m = FS.frame_fragment_streams(slab, off, ln)
    check_against_single_stream(slab, off, ln, m)
    assert set(m.rows[:, 7].tolist()) == {0, 1, 2, 3} and set(m.rows[:, 3].tolist()) == {0, 1, 2}
    assert (m.rows[:, 2] < ln).any() and len(set((off % 16).tolist())) > 8
    assert 1 <= min(np.bincount(m.frag_seg)[np.bincount(m.frag_seg) > 0]) and np.bincount(m.frag_seg).max() <= 15


def test_keep_slab():
    slab, off, ln = FS.keep_slab()
    m = FS.frame_fragment_streams(slab, off, ln)
    check_against_single_stream(slab, off, ln, m)
    for i, (walked, last_at) in enumerate(FS.KEEP_CASES):
        s = 2 * i
        assert int(m.rows[s, 1]) == last_at and int(m.rows[s, 3]) == FS.OK
        assert FR.frame_fragments(slab[int(off[s]):int(off[s] + ln[s])])[1] == walked
        assert (int(m.rows[s, 2]) == int(ln[s])) == (walked == last_at)
    assert {15, 16, 17, 32, 33} <= {w for w, _ in FS.KEEP_CASES}
    assert {15, 16, 17} <= {l for w, l in FS.KEEP_CASES if w > l}
    s = 2 * FS.KEEP_CASES.index((20, 0))
    assert tuple(int(x) for x in m.rows[s, 1:4]) == (0, 0, 0) and int(m.rows[s, 7]) == 0


def test_empties_slab():
    slab, off, ln = FS.empties_slab()
    m = FS.frame_fragment_streams(slab, off, ln)
    check_against_single_stream(slab, off, ln, m)
    assert m.rows[:, 1].tolist() == [1, 3, 5, 11, 0, 1, 0, 19] and m.rows[:, 7].tolist() == [1, 3, 1, 4, 0, 1, 0, 2]
    assert (m.rows[:, 3] == 0).all() and int(m.rows[4, 2]) == 0 and int(m.rows[5, 2]) == 4
    d = FS.defragment_extents(slab, m.frag_start, m.frag_len)
    assert d["records"][4] == FS.EMPTY and int(d["result"][0]) == 12


def test_aligned_slab():
    slab, off, ln = FS.aligned_slab()
    m = FS.frame_fragment_streams(slab, off, ln)
    check_against_single_stream(slab, off, ln, m)
    assert (off % 16).tolist() == list(range(16)) and int(off[-1] + ln[-1]) == len(slab)
    assert (m.rows[:, 1] == 6).all() and (m.rows[:, 7] == 3).all()


def test_capacity_slabs():
    slab, off, ln = FS.capacity_slab()
    full = FS.frame_fragment_streams(slab, off, ln)
    assert full.rows[:, 1].tolist() == [5, 4, 3] and int(full.result[1]) == 12 and int(full.result[3]) == 1
    check_capacities(slab, off, ln, full)
    m = FS.frame_fragment_streams(slab, off, ln, 7)          # the 4-fragment record straddles the capacity
    assert m.result.tolist() == [5, 12, 2, 0] and m.rows[1].tolist() == [5, 0, 0, 0, 0, 0, 2, 0]
    assert m.rows[2].tolist() == [7, 0, 0, 0, 0, 0, 0, 0]
    slab, off, ln = FS.long_capacity_slab()
    full = FS.frame_fragment_streams(slab, off, ln)
    assert full.rows[:, 1].tolist() == [2, 35, 3] and int(full.rows[1, 7]) == 5
    check_capacities(slab, off, ln, full)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_defragment_extents_is_defragment_of_the_concatenation(order):
    stream = FR.shapes_stream("tiny") + FR.pending_stream()[0]
    wire, start, flen = FS.scatter(stream, order)
    fo = FR.frame_fragments(stream)[0]
    C, off = FS.concat_extents(wire, start, flen)
    assert C == stream and np.array_equal(off, fo)
    if order == "descending":
        assert (np.diff(start.astype(np.int64)) < 0).all()
    want = FR.defragment(stream, fo)
    got = FS.defragment_extents(wire, start, flen)
    assert got["records"] == want["records"] and np.array_equal(got["rec_off"], want["rec_off"])
    assert int(want["result"][3]) == 3 and int(got["result"][1]) == len(start) - 3
    assert np.array_equal(np.delete(got["result"], 1), np.delete(want["result"], 1))
    cap = int(want["rec_off"][5]) + 2
    cut = FS.defragment_extents(wire, start, flen, cap)
    assert cut["status"].tolist()[:6] == [0, 0, 0, 0, 0, FR.ENC_WRITE_ZERO]
