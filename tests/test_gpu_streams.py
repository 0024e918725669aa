"""Segmented framing on the GPU (onc_frame_streams, streams.hip) against the
host model of its serial loop (tests/streams_model.py, itself checked against
the oracle's per-segment expected_message_len loop in
tests/test_streams_model.py). Every comparison is bit-exact: rec_start,
rec_len, rec_seg, all six words of every segment row, and result; entries of
the record arrays at or past result[0] must keep the filler they had.

Between segments the slabs hold bytes that read as record marks, so a framer
that leaves a segment fails by comparison. No segment list points outside its
slab."""
import numpy as np
import pytest

import frame_model as FM
import onc_rpc_amd.layout as L
import streams_model as SM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codec(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = R.Codec(0)
    yield c
    c.close()


def _i64(a):
    import torch
    return torch.from_numpy(np.append(np.ascontiguousarray(a, np.uint64), np.uint64(0)).view(np.int64).copy()).cuda()


class Run:
    """One onc_frame_streams call with sentinel-filled outputs."""

    def __init__(self, codec, wire, off, ln, cap, with_seg=True, room=None):
        import torch
        nseg = len(off)
        room = (cap if room is None else room) + 3
        self.start = torch.full((room,), -1, dtype=torch.int64, device="cuda")
        self.len = torch.full((room,), -1, dtype=torch.int32, device="cuda")
        self.seg = torch.full((room,), -1, dtype=torch.int32, device="cuda") if with_seg else None
        self.rows = torch.full((6 * nseg + 2,), -1, dtype=torch.int64, device="cuda")
        self.res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        self.off, self.ln = _i64(off), _i64(ln)
        self.nseg, self.cap = nseg, cap
        self.args = (wire, self.off, self.ln, nseg, self.start, self.len, self.seg, cap, self.rows, self.res)
        codec.frame_streams(*self.args)
        codec.sync()

    def check(self, want: SM.Framed, what=""):
        res = self.res.cpu().numpy().view(np.uint64)
        assert np.array_equal(res[:3], want.result), f"{what}: result {res[:3]} != {want.result}"
        assert res[3] == np.uint64(2**64 - 1)
        rows = self.rows.cpu().numpy().view(np.uint64)
        got = rows[:6 * self.nseg].reshape(-1, 6)
        bad = np.nonzero((got != want.rows).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: rows differ at {bad[:8]}: {got[bad[0]]} != {want.rows[bad[0]]}"
        assert (rows[6 * self.nseg:] == np.uint64(2**64 - 1)).all()
        n = int(want.result[0])
        start = self.start.cpu().numpy().view(np.uint64)
        ln = self.len.cpu().numpy().view(np.uint32)
        assert np.array_equal(start[:n], want.rec_start), f"{what}: rec_start"
        assert np.array_equal(ln[:n], want.rec_len), f"{what}: rec_len"
        assert (start[n:] == np.uint64(2**64 - 1)).all() and (ln[n:] == 0xFFFFFFFF).all(), f"{what}: written past n"
        if self.seg is not None:
            seg = self.seg.cpu().numpy().view(np.uint32)
            assert np.array_equal(seg[:n], want.rec_seg), f"{what}: rec_seg"
            assert (seg[n:] == 0xFFFFFFFF).all()


def _dev(R, slab):
    return R.to_device(np.frombuffer(bytes(slab), np.uint8), "cuda")


def _case(R, codec, slab, off, ln, cap=None, what="", **kw):
    want = SM.frame_streams(slab, off, ln, cap)
    room = int(want.result[1]) + 5
    Run(codec, _dev(R, slab), off, ln, room if cap is None else cap, room=max(room, cap or 0), **kw).check(want, what)
    return want


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["edge", "cut", "cut short"])
def test_one_segment_is_frame_stream(R, codec, which):
    buf = {"edge": FM.edge_stream, "cut": FM.cut_stream}.get(which, FM.cut_stream)()
    if which == "cut short":
        buf = buf[:-7]
    want = _case(R, codec, buf, [0], [len(buf)], what=which)
    off, n, consumed, st, a0, a1 = R.frame_host_stream(codec, buf)
    assert np.array_equal(off[:n], want.rec_start)
    assert np.array_equal(np.diff(off.astype(np.int64)), want.rec_len.astype(np.int64))
    assert tuple(int(x) for x in want.rows[0]) == (0, n, consumed, st, a0, a1)
    if which == "cut short":
        assert st == SM.INCOMPLETE_MESSAGE


@pytest.mark.parametrize("nseg", [63, 64, 65, 129, 257])
def test_small_segments(R, codec, nseg):
    """Wave (64), write workgroup (16) and scan-tile (256) edges."""
    slab, off, ln = SM.small_segments(nseg)
    _case(R, codec, slab, off, ln, what=f"nseg {nseg}")


def test_66000_segments(R, codec):
    slab, off, ln = SM.reply_segments()
    want = _case(R, codec, slab, off, ln, what="66000 segments")
    assert len(off) > 65_536 and int(want.result[0]) > 60_000


def test_stops_leave_neighbours_alone(R, codec):
    slab, off, ln, where = SM.stops_slab()
    want = _case(R, codec, slab, off, ln, what="stops")
    assert tuple(int(x) for x in want.rows[where["all ones"], 3:]) == (SM.INCOMPLETE_MESSAGE, 8, 0x80000003)
    assert int(want.result[2]) == 7


def test_bare_marks_kept_and_rechased(R, codec):
    slab, off, ln = SM.marks_slab()
    want = _case(R, codec, slab, off, ln, what="bare marks")
    assert want.rows[0::2, 1].tolist() == list(SM.MARK_COUNTS)


def test_one_mebibyte_segment(R, codec):
    slab, off, ln = SM.long_slab()
    want = _case(R, codec, slab, off, ln, what="1 MiB segment")
    assert int(want.rows[1, 1]) > 5000


def test_sixteen_alignments(R, codec):
    slab, off, ln = SM.aligned_slab()
    assert (off % 16).tolist() == list(range(16))
    _case(R, codec, slab, off, ln, what="alignments")


def test_descending_and_repeated_segments(R, codec):
    slab, off, ln = SM.small_segments(129)
    _case(R, codec, slab, off[::-1].copy(), ln[::-1].copy(), what="descending")
    _case(R, codec, slab, np.concatenate([off, off]), np.concatenate([ln, ln]), what="listed twice")
    # overlapping: the second segment starts at the first one's second record
    w = SM.frame_streams(slab, off, ln)
    s = int(np.nonzero(w.rows[:, 1] >= 2)[0][0])
    k = int(w.rows[s, 0])
    o2 = np.array([off[s], w.rec_start[k + 1]], np.uint64)
    l2 = np.array([ln[s], off[s] + ln[s] - w.rec_start[k + 1]], np.uint64)
    _case(R, codec, slab, o2, l2, what="overlapping")


def test_rec_seg_null(R, codec):
    slab, off, ln = SM.small_segments(65)
    _case(R, codec, slab, off, ln, what="rec_seg NULL", with_seg=False)


def test_segment_ends_on_the_allocations_last_byte(R, codec):
    """A mapped host slab of exactly two pages whose last segment ends with a
    bare mark on the mapping's last four bytes, and one whose last segment ends
    with a cut three-byte tail there."""
    for tail in (b"\x80\x00\x00\x00", b"\x80\x00\x00"):
        seg = FM.reply28(5) + FM.reply(6, b"\x02" * 7) + tail
        body = SM.GAP * ((8192 - len(seg)) // 4 + 1)
        slab = body[:8192 - len(seg)] + seg
        assert len(slab) == 8192
        off = np.array([16, 8192 - len(seg)], np.uint64)
        ln = np.array([28, len(seg)], np.uint64)
        want = SM.frame_streams(slab, off, ln)
        assert int(want.rows[1, 2]) == (len(seg) if len(tail) == 4 else len(seg) - 3)
        m = R.HostMapped.from_array(codec, np.frombuffer(slab, np.uint8))
        try:
            Run(codec, m, off, ln, 8).check(want, "last byte")
        finally:
            m.close()


def test_capacity(R, codec):
    from test_streams_model import capacity_values
    slab, off, ln = SM.capacity_slab()
    full, caps = capacity_values(slab, off, ln)
    needed = int(full.result[1])
    w = _dev(R, slab)
    for cap in caps:
        want = SM.frame_streams(slab, off, ln, cap)
        assert int(want.result[1]) == (needed if cap else 0)
        Run(codec, w, off, ln, cap, room=needed + 5).check(want, f"max_records {cap}")


def test_no_segments(R, codec):
    import torch
    res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    codec.frame_streams(None, None, None, 0, None, None, None, 10, None, res)
    codec.sync()
    assert not res.cpu().numpy().any()


def test_pinned_host_slab(R, codec):
    slab, off, ln = SM.connection_slab()
    want = SM.frame_streams(slab, off, ln)
    m = R.HostMapped.from_array(codec, np.frombuffer(slab, np.uint8))
    try:
        Run(codec, m, off, ln, int(want.result[1]) + 5).check(want, "mapped host slab")
    finally:
        m.close()


def test_graph_capture_frame_then_decode(R, oracle):
    """onc_codec_reserve, then frame_streams + decode_extents captured on the
    codec's stream (one chain of kernels) and replayed on two other slabs
    copied into the same buffer. The decode runs over max_records extents:
    those past result[0] are what the caller left there (empty records here)."""
    import torch
    from test_gpu_extents import expect_extents
    from test_gpu_parity import assert_decoded_equal
    slabs = [SM.connection_slab(100, seed) for seed in (13, 14, 15)]
    size = max(len(s[0]) for s in slabs)
    cap = 4096
    s = torch.cuda.Stream()
    c = R.Codec(0, stream=s.cuda_stream, decode_policy=R.DECODE_POLICY_STANDARD)
    try:
        wire = torch.zeros(size, dtype=torch.uint8, device="cuda")
        off, ln = _i64(slabs[0][1]), _i64(slabs[0][2])
        start = torch.zeros(cap, dtype=torch.int64, device="cuda")
        rlen = torch.zeros(cap, dtype=torch.int32, device="cuda")
        rows = torch.zeros(600, dtype=torch.int64, device="cuda")
        res = torch.zeros(3, dtype=torch.int64, device="cuda")
        d = R.DecodeBuffers(cap)

        def work():
            c.frame_streams(wire, off, ln, 100, start, rlen, None, cap, rows, res)
            c.decode_extents(wire, size, start, rlen, cap, L.DECODE_SLICE, d.msgs, d.unix, d.status, d.aux0, d.aux1)

        # without the reserve, the framer would grow its scratch inside the capture
        g0 = torch.cuda.CUDAGraph()
        err = None
        with torch.cuda.graph(g0, stream=s):
            try:
                c.frame_streams(wire, off, ln, 100, start, rlen, None, cap, rows, res)
            except R.CodecError as e:
                err = str(e)
        assert err is not None and "rc=-5" in err, err
        c.reserve(cap)
        wire[:len(slabs[0][0])] = torch.from_numpy(np.frombuffer(slabs[0][0], np.uint8).copy()).cuda()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            work()                                   # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            work()
        torch.cuda.synchronize()
        for slab, so, sl in slabs[1:]:
            wire[:len(slab)] = torch.from_numpy(np.frombuffer(slab, np.uint8).copy()).cuda()
            ln.copy_(_i64(sl))
            start.zero_()
            rlen.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = SM.frame_streams(slab, so, sl, cap)
            n = int(want.result[0])
            assert 0 < n < cap
            assert np.array_equal(res.cpu().numpy().view(np.uint64), want.result)
            assert np.array_equal(rows.cpu().numpy().view(np.uint64).reshape(-1, 6), want.rows)
            assert np.array_equal(start.cpu().numpy().view(np.uint64)[:n], want.rec_start)
            assert np.array_equal(rlen.cpu().numpy().view(np.uint32)[:n], want.rec_len)
            assert not start.cpu().numpy()[n:].any() and not rlen.cpu().numpy()[n:].any()
            host = np.frombuffer(slab, np.uint8)
            exp = expect_extents(oracle, host, np.append(want.rec_start, np.zeros(cap - n, np.uint64)),
                                 np.append(want.rec_len, np.zeros(cap - n, np.uint32)), len(host), L.DECODE_SLICE)
            assert_decoded_equal(d.to_host(), exp[:5], "replayed frame + decode")
    finally:
        c.close()
