"""Fragmented records of many connections on the GPU:
onc_frame_fragment_streams (streams.hip fragstreams_*) and
onc_defragment_extents (defrag.hip, extents form) against their host models
(tests/fragment_streams_model.py, itself checked against the single-stream
models in tests/test_fragment_streams_model.py), against the library's own
single-stream pair, and end to end against the oracle's decode of the
original unfragmented records. Every comparison is bit-exact: the extents, all
eight words of every segment row, result; rec_off, status, result and every
output byte of the reassembly, guards included. Entries at or past result[0]
must keep the filler they had.

Between segments the slabs hold bytes that read as record marks, so a framer
that leaves a segment fails by comparison. No segment or extent list points
outside its buffer."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fragment_model as FR
import fragment_streams_model as FS
import frame_model as FM
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
import streams_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
U64 = np.uint64(2**64 - 1)
SENT, GUARD = 0xA5, 64


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codec(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)
    yield c
    c.close()


def _i64(a):
    import torch
    return torch.from_numpy(np.append(np.ascontiguousarray(a, np.uint64), np.uint64(0)).view(np.int64).copy()).cuda()


def _i32(a):
    import torch
    return torch.from_numpy(np.append(np.ascontiguousarray(a, np.uint32), np.uint32(0)).view(np.int32).copy()).cuda()


def _dev(R, slab):
    return R.to_device(np.frombuffer(bytes(slab), np.uint8), "cuda")


class Run:
    """One onc_frame_fragment_streams call with sentinel-filled outputs."""

    def __init__(self, codec, wire, off, ln, cap, with_seg=True, room=None):
        import torch
        nseg = len(off)
        room = (cap if room is None else room) + 3
        self.start = torch.full((room,), -1, dtype=torch.int64, device="cuda")
        self.len = torch.full((room,), -1, dtype=torch.int32, device="cuda")
        self.seg = torch.full((room,), -1, dtype=torch.int32, device="cuda") if with_seg else None
        self.rows = torch.full((8 * nseg + 2,), -1, dtype=torch.int64, device="cuda")
        self.res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        self.off, self.ln = _i64(off), _i64(ln)
        self.nseg = nseg
        codec.frame_fragment_streams(wire, self.off, self.ln, nseg, self.start, self.len, self.seg, cap, self.rows,
                                     self.res)
        codec.sync()

    def check(self, want: FS.Fragged, what=""):
        res = self.res.cpu().numpy().view(np.uint64)
        assert np.array_equal(res[:4], want.result), f"{what}: result {res[:4]} != {want.result}"
        assert res[4] == U64
        rows = self.rows.cpu().numpy().view(np.uint64)
        got = rows[:8 * self.nseg].reshape(-1, 8)
        bad = np.nonzero((got != want.rows).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: rows differ at {bad[:8]}: {got[bad[0]]} != {want.rows[bad[0]]}"
        assert (rows[8 * self.nseg:] == U64).all()
        n = int(want.result[0])
        start = self.start.cpu().numpy().view(np.uint64)
        ln = self.len.cpu().numpy().view(np.uint32)
        assert np.array_equal(start[:n], want.frag_start), f"{what}: frag_start"
        assert np.array_equal(ln[:n], want.frag_len), f"{what}: frag_len"
        assert (start[n:] == U64).all() and (ln[n:] == 0xFFFFFFFF).all(), f"{what}: written past n"
        if self.seg is not None:
            seg = self.seg.cpu().numpy().view(np.uint32)
            assert np.array_equal(seg[:n], want.frag_seg), f"{what}: frag_seg"
            assert (seg[n:] == 0xFFFFFFFF).all()


def _case(R, codec, slab, off, ln, cap=None, what="", **kw):
    want = FS.frame_fragment_streams(slab, off, ln, cap)
    room = int(want.result[1]) + 5
    Run(codec, _dev(R, slab), off, ln, room if cap is None else cap, room=max(room, cap or 0), **kw).check(want, what)
    return want


def _defrag_ext(R, codec, wire, start, flen, out_cap=None, shift=1):
    """onc_defragment_extents == the model: bytes (sentinel intact outside OK
    records, guards included), rec_off, status, result, unwritten tails.
    Returns (model, out bytes)."""
    import torch
    nfrag = len(start)
    m = FS.defragment_extents(wire, start, flen, out_cap)
    need = int(m["rec_off"][-1])
    cap = need if out_cap is None else out_cap
    w = R.to_device(np.frombuffer(bytes(wire) + b"\0" * 16, np.uint8), "cuda")
    span = max(cap, need)
    base = torch.full((GUARD + 16 + span + GUARD + 16,), SENT, dtype=torch.uint8, device="cuda")
    lo = GUARD + (-base.data_ptr() - GUARD) % 16 + shift          # out = a 16-byte aligned address + shift
    rec_off = torch.full((nfrag + 2,), -2, dtype=torch.int64, device="cuda")
    status = torch.full((nfrag + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    res = torch.full((7,), -1, dtype=torch.int64, device="cuda")
    codec.defragment_extents(w, _i64(start), _i32(flen), nfrag, base.data_ptr() + lo, rec_off, status, res, out_cap=cap)
    codec.sync()
    n = int(m["result"][0])
    r = res.cpu().numpy().view(np.uint64)
    assert r[:6].tolist() == m["result"].tolist(), (r.tolist(), m["result"].tolist())
    assert r[6] == U64
    ro = rec_off.cpu().numpy()
    assert np.array_equal(ro[:n + 1].view(np.uint64), m["rec_off"])
    assert (ro[n + 1:] == -2).all(), "rec_off written past n_records"
    st = status.cpu().numpy()
    assert st[:n].tolist() == m["status"].tolist()
    assert (st[n:] == 0x5A5A5A5A).all(), "status written from n_records on"
    got = base.cpu().numpy()
    want = np.full(got.size, SENT, np.uint8)
    want[lo:lo + span] = FR.expected_out(m, span, SENT)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"out differs first at byte {bad[0] - lo} of {need} (cap {cap}): "
                           f"{got[bad[:8]]} vs {want[bad[:8]]}")
    return m, got[lo:lo + need].tobytes()


# ---------------------------------------------------------------------------
# 1. one segment: the model and the library's single-stream pair
# ---------------------------------------------------------------------------
def _one_segment(kind):
    rng = np.random.default_rng(61)
    body = b"".join(FS.record(rng, k) for k in (1, 3, 2, 5))
    if kind.startswith("cut mark"):
        tail = FS._pending(rng, 2) + b"\x80\x00\x00\x10"[:int(kind[-1])]
    else:
        tail = FS.ending(rng, kind)[0]
    return body + tail, len(body)


@pytest.mark.parametrize("kind", ["clean", "cut fragment", "cut mark 1", "cut mark 2", "cut mark 3", "pending"])
def test_one_segment_is_frame_fragments_and_defragment(R, codec, kind):
    buf, whole = _one_segment(kind)
    want = _case(R, codec, buf, [0], [len(buf)], what=kind)
    fo, nf, consumed, st, a0, a1 = R.frame_host_fragments(codec, buf)
    rb, ro, rs, rr, _ = R.reassemble_host_stream(codec, buf)
    pending = int(rr[3])
    assert tuple(int(x) for x in want.rows[0]) == (0, nf - pending, int(rr[1]), st, a0, a1, 0, int(rr[0]))
    assert int(want.rows[0, 2]) == whole and int(want.rows[0, 7]) == 4
    assert st == {"clean": 0, "pending": 0, "cut fragment": 1}.get(kind, 2)
    assert np.array_equal(want.frag_start, fo[:nf - pending])
    m, got = _defrag_ext(R, codec, buf, want.frag_start, want.frag_len)
    assert got == rb and np.array_equal(m["rec_off"], ro) and not rs.any()
    assert m["result"].tolist() == [int(rr[0]), nf - pending, int(rr[2]), 0, 0, int(rr[5])]


# ---------------------------------------------------------------------------
# 2. many segments; the kept / re-chased boundary; empties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", [63, 64, 65, 129, 257])
def test_random_segments(R, codec, nseg):
    """Chase workgroup (64 segments), write workgroup (16) and scan-tile (256) edges."""
    slab, off, ln = FS.random_segments(nseg)
    want = _case(R, codec, slab, off, ln, what=f"nseg {nseg}")
    assert set(want.rows[:, 3].tolist()) == {0, 1, 2}
    _defrag_ext(R, codec, slab, want.frag_start, want.frag_len, shift=nseg % 16)


def test_kept_and_rechased_segments(R, codec):
    slab, off, ln = FS.keep_slab()
    want = _case(R, codec, slab, off, ln, what="keep boundary")
    assert want.rows[0::2, 1].tolist() == [l for _, l in FS.KEEP_CASES]
    s = 2 * FS.KEEP_CASES.index((20, 0))                    # 20 fragments, all pending
    assert tuple(int(x) for x in want.rows[s, 1:4]) == (0, 0, 0)
    _defrag_ext(R, codec, slab, want.frag_start, want.frag_len)


def test_empty_fragments_and_records(R, codec):
    slab, off, ln = FS.empties_slab()
    want = _case(R, codec, slab, off, ln, what="empties")
    assert int(want.result[2]) == 12
    m, _ = _defrag_ext(R, codec, slab, want.frag_start, want.frag_len)
    assert m["records"][4] == FS.EMPTY


# ---------------------------------------------------------------------------
# 3. where the segments lie
# ---------------------------------------------------------------------------
def test_sixteen_alignments_and_a_tight_end(R, codec):
    slab, off, ln = FS.aligned_slab()
    assert (off % 16).tolist() == list(range(16)) and int(off[-1] + ln[-1]) == len(slab)
    _case(R, codec, slab, off, ln, what="alignments")


def test_descending_repeated_and_no_frag_seg(R, codec):
    slab, off, ln = FS.random_segments(129)
    _case(R, codec, slab, off[::-1].copy(), ln[::-1].copy(), what="descending")
    _case(R, codec, slab, np.concatenate([off, off]), np.concatenate([ln, ln]), what="listed twice")
    _case(R, codec, slab, off, ln, what="frag_seg NULL", with_seg=False)


def test_segment_ends_on_the_allocations_last_byte(R, codec):
    """A mapped host slab of exactly two pages whose last segment ends with a
    bare last mark on the mapping's last four bytes, and one whose last segment
    ends with a cut three-byte tail there."""
    rng = np.random.default_rng(63)
    for tail in (FS.EMPTY, b"\x00\x00\x00"):
        seg = FS.record(rng, 3) + FS.CONT0 + tail
        body = SM.GAP * ((8192 - len(seg)) // 4 + 1)
        slab = body[:8192 - len(seg)] + seg
        assert len(slab) == 8192
        off = np.array([16, 8192 - len(seg)], np.uint64)
        ln = np.array([28, len(seg)], np.uint64)
        want = FS.frame_fragment_streams(slab, off, ln)
        assert int(want.rows[1, 2]) == (len(seg) if len(tail) == 4 else len(seg) - 7)
        m = R.HostMapped.from_array(codec, np.frombuffer(slab, np.uint8))
        try:
            Run(codec, m, off, ln, 16).check(want, "last byte")
        finally:
            m.close()


# ---------------------------------------------------------------------------
# 4. capacity
# ---------------------------------------------------------------------------
def test_every_capacity_of_a_small_slab(R, codec):
    slab, off, ln = FS.capacity_slab()
    w = _dev(R, slab)
    needed = int(FS.frame_fragment_streams(slab, off, ln).result[1])
    assert needed == 12
    for cap in range(0, needed + 2):
        want = FS.frame_fragment_streams(slab, off, ln, cap)
        Run(codec, w, off, ln, cap, room=needed + 5).check(want, f"max_frags {cap}")
    want = FS.frame_fragment_streams(slab, off, ln, 7)       # a record's fragments straddle the capacity
    assert want.result.tolist() == [5, 12, 2, 0] and want.rows[2].tolist() == [7, 0, 0, 0, 0, 0, 0, 0]


def test_capacity_cuts_a_rechased_segment(R, codec):
    slab, off, ln = FS.long_capacity_slab()
    w = _dev(R, slab)
    needed = int(FS.frame_fragment_streams(slab, off, ln).result[1])
    assert needed == 40
    for cap in (1, 2, 3, 8, 9, 15, 16, 17, 18, 22, 23, 36, 37, 39, 40, 41):
        want = FS.frame_fragment_streams(slab, off, ln, cap)
        Run(codec, w, off, ln, cap, room=needed + 5).check(want, f"max_frags {cap}")


def test_no_segments_and_no_capacity(R, codec):
    import torch
    res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    codec.frame_fragment_streams(None, None, None, 0, None, None, None, 10, None, res)
    codec.sync()
    assert not res.cpu().numpy().any()
    slab, off, ln = FS.capacity_slab()
    Run(codec, _dev(R, slab), off, ln, 0, room=4).check(FS.frame_fragment_streams(slab, off, ln, 0), "max_frags 0")


# ---------------------------------------------------------------------------
# 5. a stopped or pending segment changes nothing outside its own row
# ---------------------------------------------------------------------------
def test_stopped_segment_leaves_neighbours_alone(R, codec):
    rng = np.random.default_rng(65)
    healthy = [b"".join(FS.record(rng, k) for k in ks) for ks in ((2, 1), (3,), (1, 1, 4), (2, 2))]
    mid = FS.record(rng, 2) + FS.record(rng, 3)
    base = None
    for kind in FS.ENDINGS:
        sl = SM.Slab(front=6)
        sl.add(healthy[0], gap=3)
        sl.add(healthy[1], gap=5)
        sl.add(mid + FS.ending(np.random.default_rng(66), kind)[0], gap=64)
        sl.add(healthy[2], gap=1)
        sl.add(healthy[3], gap=2)
        slab, off, ln = sl.done()
        want = _case(R, codec, slab, off, ln, what=kind)
        assert int(want.rows[2, 3]) == {"clean": 0, "pending": 0, "cut mark": 2, "cut fragment": 1}[kind]
        assert tuple(int(x) for x in want.rows[2, [1, 2, 7]]) == (5, len(mid), 2)
        others = want.rows[[0, 1, 3, 4]][:, [0, 1, 2, 3, 6, 7]]
        base = others if base is None else base
        assert np.array_equal(others, base), kind


# ---------------------------------------------------------------------------
# 6. onc_defragment_extents
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shift", range(16))
def test_defragment_every_out_alignment(R, codec, shift):
    wire, start, flen = FS.scatter(FR.alignment_stream(reps=1), "shuffled", seed=70 + shift)
    m, got = _defrag_ext(R, codec, wire, start, flen, shift=shift)
    buf = FR.alignment_stream(reps=1)
    assert got == b"".join(FR.defragment(buf, FR.frame_fragments(buf)[0])["records"])


def test_defragment_capacity_cuts_mid_batch(R, codec):
    wire, start, flen = FS.scatter(FR.shapes_stream("tiny"), "ascending")
    full = FS.defragment_extents(wire, start, flen)
    n = int(full["result"][0])
    for r in (1, n // 2, n):
        end = int(full["rec_off"][r])
        for cap in (end - 1, end):
            m, _ = _defrag_ext(R, codec, wire, start, flen, out_cap=cap)
            assert m["status"].tolist() == [0 if int(e) <= cap else FR.ENC_WRITE_ZERO for e in full["rec_off"][1:]]
    m, _ = _defrag_ext(R, codec, wire, start, flen, out_cap=0)
    assert m["status"].tolist() == [FR.ENC_WRITE_ZERO] * n


def test_defragment_record_spanning_the_plan_block(R, codec):
    """300 fragments: a record of 30 fragments lies across fragment 256."""
    rng = np.random.default_rng(71)
    stream = b"".join(FS.record(rng, 1) for _ in range(240)) + FS.record(rng, 30, max_body=400) \
        + b"".join(FS.record(rng, 3) for _ in range(10))
    fo = FR.frame_fragments(stream)[0]
    assert len(fo) - 1 == 300
    wire, start, flen = FS.scatter(stream, "shuffled")
    m, got = _defrag_ext(R, codec, wire, start, flen, shift=3)
    assert int(m["result"][0]) == 251 and got == b"".join(FR.defragment(stream, fo)["records"])


def test_defragment_more_fragments_in_a_tile_than_the_stage(R, codec):
    """200 one-byte or empty fragments inside one 8 KiB output tile (kDfStage is 128)."""
    rng = np.random.default_rng(72)
    lens = rng.integers(0, 2, 200)
    body = rng.bytes(int(lens.sum()))
    stream = FM.opaque(rng.bytes(300)) + FR.fragment(body, np.cumsum(lens)[:-1].tolist()) + FM.opaque(rng.bytes(500))
    assert len(stream) < FR.TILE and FR.fragments_per_record(stream).max() == 200 > FR.STAGE
    for order in ("ascending", "shuffled"):
        wire, start, flen = FS.scatter(stream, order)
        _, got = _defrag_ext(R, codec, wire, start, flen, shift=5)
        assert got[-504:] == stream[-504:]


def test_defragment_descending_addresses_and_pending_extents(R, codec):
    stream, head = FR.pending_stream()
    wire, start, flen = FS.scatter(stream, "descending")
    assert (np.diff(start.astype(np.int64)) < 0).all()
    m, got = _defrag_ext(R, codec, wire, start, flen)
    nfrag = len(start)
    assert m["result"].tolist() == [3, nfrag - 3, int(m["rec_off"][3]), 3, 90, 1]
    assert got == b"".join(FR.defragment(stream, FR.frame_fragments(stream)[0])["records"])
    # only pending extents; nothing at all
    m, _ = _defrag_ext(R, codec, wire, start[-3:], flen[-3:])
    assert m["result"].tolist() == [0, 0, 0, 3, 90, 0]
    _defrag_ext(R, codec, wire, start[:0], flen[:0])


# ---------------------------------------------------------------------------
# 7. the mixed server, end to end
# ---------------------------------------------------------------------------
NCONN = 130


class Server:
    """NCONN connections' buffers in one slab, built from oracle-encoded
    records: every fourth connection's peer fragments its records, some
    connections end in a cut tail. Keeps what every connection's whole records
    are (the original unfragmented bytes)."""

    def __init__(self, oracle, seed=81):
        rng = np.random.default_rng(seed)
        wire, off, st, _ = oracle.encode_batch(L.build_batch(S.random_messages(700, seed=seed, max_payload=300)))
        assert not st.any()
        recs = [wire[int(off[i]):int(off[i + 1])] for i in range(700)]
        cuts = FR.random_cuts(seed)
        sl = SM.Slab(front=int(rng.integers(0, 16)))
        self.orig, self.fragmenting, self.whole_len = [], [], []
        r = 0
        for c in range(NCONN):
            k = int(rng.integers(0, 6))
            mine, r = recs[r:r + k], r + k
            frag = c % 4 == 1

            def on_wire(rec):
                return FR.fragment(rec[4:], cuts(0, len(rec) - 4)) if frag else rec
            data = b"".join(on_wire(x) for x in mine)
            self.whole_len.append(len(data))
            if c % 3 == 0:                                 # a cut tail: part of the next record, as it is on the wire
                nxt = on_wire(recs[r])
                r += 1
                data += nxt[:int(rng.integers(1, len(nxt)))]
            self.orig.append(mine)
            self.fragmenting.append(frag)
            sl.add(data, gap=int(rng.integers(0, 24)))
        assert r <= 700
        self.slab, self.off, self.len = sl.done()


@pytest.fixture(scope="module")
def server(oracle):
    return Server(oracle)


def _oracle_decode(oracle, recs, mode):
    w, o = b"".join(recs), np.concatenate(([0], np.cumsum([len(x) for x in recs]))).astype(np.uint64)
    return oracle.decode_batch(np.frombuffer(w + b"\0" * 16, np.uint8).copy(), o, mode), w, o


def _defrag_mapped(codec, wire, d_start, d_len, nfrag, cap):
    """onc_defragment_extents reading the fragments where `wire` lies, from
    extents already on the device -> (bytes, rec_off, status, result)."""
    import torch
    out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    rec_off = torch.zeros(nfrag + 1, dtype=torch.int64, device="cuda")
    status = torch.zeros(max(nfrag, 1), dtype=torch.int32, device="cuda")
    res = torch.zeros(6, dtype=torch.int64, device="cuda")
    codec.defragment_extents(wire, d_start, d_len, nfrag, out, rec_off, status, res, out_cap=cap)
    codec.sync()
    r = res.cpu().numpy().view(np.uint64).copy()
    n = int(r[0])
    return (out.cpu().numpy()[:int(r[2])].tobytes(), rec_off.cpu().numpy().view(np.uint64)[:n + 1].copy(),
            status.cpu().numpy()[:n].copy(), r)


def _mixed_flow(R, codec, oracle, srv, slab_dev=None):
    """onc_frame_streams on the slab, the rests of the FRAGMENTED rows through
    the new calls, onc_decode of the rebuilt stream. Checks every connection's
    results, in order, against the oracle's decode of its original records."""
    from test_gpu_extents import expect_extents
    from test_gpu_bounded import check
    from test_gpu_parity import assert_decoded_equal
    slab, off, ln = srv.slab, srv.off, srv.len
    host = np.frombuffer(slab, np.uint8)
    start, length, seg, rows, res = R.frame_host_streams(codec, slab, off, ln)
    fragd = np.nonzero(rows[:, 3] == SM.FRAGMENTED)[0]
    assert 15 <= len(fragd) and all(srv.fragmenting[c] for c in fragd)
    roff = off[fragd] + rows[fragd, 2]
    rlen = ln[fragd] - rows[fragd, 2]
    want = FS.frame_fragment_streams(slab, roff, rlen)
    if slab_dev is None:
        rb, ro, rs, rrows, fres, dres = R.reassemble_host_streams(codec, slab, roff, rlen)
    else:                                                   # the slab where it lies (mapped host memory)
        run = Run(codec, slab_dev, roff, rlen, int(want.result[1]) + 5)
        run.check(want, "mapped slab")
        rb, ro, rs, dres = _defrag_mapped(codec, slab_dev, run.start, run.len, int(want.result[0]), len(slab))
        rrows, fres = want.rows, want.result
    assert np.array_equal(rrows, want.rows) and np.array_equal(fres, want.result)
    assert not rs.any() and int(dres[3]) == 0 and int(dres[1]) == int(fres[0])
    # per connection, in order: in-place records, then rebuilt ones = its original records
    j_of = {int(c): j for j, c in enumerate(fragd)}
    rebuilt_expect = []
    for c in range(NCONN):
        n1 = int(rows[c, 1])
        n2 = int(rrows[j_of[c], 7]) if c in j_of else 0
        assert n1 + n2 == len(srv.orig[c]), c
        consumed = int(rows[c, 2]) + (int(rrows[j_of[c], 2]) if c in j_of else 0)
        assert consumed == srv.whole_len[c], c
        k = int(rows[c, 0])
        for i in range(n1):
            assert slab[int(start[k + i]):int(start[k + i]) + int(length[k + i])] == srv.orig[c][i]
        if c in j_of:
            assert int(rrows[j_of[c], 6]) == len(rebuilt_expect)
            rebuilt_expect += srv.orig[c][n1:]
    assert int(dres[5]) > 10                               # records that came in more than one fragment
    for mode in MODES:
        got = R.decode_host_extents(codec, host, start, length, mode)
        check(got, expect_extents(oracle, host, start, length, len(host), mode), f"in place, mode {mode}")
        exp, w, o = _oracle_decode(oracle, rebuilt_expect, mode)
        assert rb == w and np.array_equal(ro, o)             # payload bytes included
        g = R.decode_host_wire(codec, np.frombuffer(rb + b"\0" * 16, np.uint8).copy(), ro, mode)
        assert_decoded_equal(g, exp, f"rebuilt, mode {mode}")


def test_mixed_server_end_to_end(R, codec, oracle, server):
    _mixed_flow(R, codec, oracle, server)


def test_fragmented_slab_in_pinned_host_memory(R, codec, oracle, server):
    m = R.HostMapped.from_array(codec, np.frombuffer(server.slab, np.uint8))
    try:
        _mixed_flow(R, codec, oracle, server, slab_dev=m)
    finally:
        m.close()


# ---------------------------------------------------------------------------
# 8. graph capture
# ---------------------------------------------------------------------------
def test_graph_capture_frame_defragment_decode(R, oracle):
    """onc_codec_reserve, then frame_fragment_streams + defragment_extents +
    decode captured on the codec's stream and replayed on two other slabs
    copied into the same buffer. The captured calls run over `cap` extents and
    records: the extents past result[0] are what the caller left there (a
    pending empty fragment kept at the buffer's end), the offsets past
    n_records too (the output's capacity: empty records at its end)."""
    import torch
    from test_gpu_parity import assert_decoded_equal
    servers = [Server(oracle, seed) for seed in (82, 83, 84)]
    lists = []
    for srv in servers:                                      # every connection goes through the fragment path
        lists.append((srv.slab, srv.off, srv.len, FS.frame_fragment_streams(srv.slab, srv.off, srv.len)))
    size = max(len(x[0]) for x in lists) + 16
    cap, out_cap = 4096, size
    s = torch.cuda.Stream()
    c = R.Codec(0, stream=s.cuda_stream, decode_policy=R.DECODE_POLICY_STANDARD)
    try:
        wire = torch.zeros(size + 32, dtype=torch.uint8, device="cuda")      # [size, size + 4): 00 00 00 00
        off, ln = _i64(lists[0][1]), _i64(lists[0][2])
        start = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
        flen = torch.zeros(cap + 1, dtype=torch.int32, device="cuda")
        rows = torch.zeros(8 * NCONN, dtype=torch.int64, device="cuda")
        fres = torch.zeros(4, dtype=torch.int64, device="cuda")
        out = torch.zeros(out_cap + 64, dtype=torch.uint8, device="cuda")
        rec_off = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
        status = torch.zeros(cap, dtype=torch.int32, device="cuda")
        dres = torch.zeros(6, dtype=torch.int64, device="cuda")
        d = R.DecodeBuffers(cap)

        def work():
            c.frame_fragment_streams(wire, off, ln, NCONN, start, flen, None, cap, rows, fres)
            c.defragment_extents(wire, start, flen, cap, out, rec_off, status, dres, out_cap=out_cap)
            c.decode(out, rec_off, cap, L.DECODE_SLICE, d.msgs, d.unix, d.status, d.aux0, d.aux1)

        def refresh(slab, sl):
            wire[:len(slab)] = torch.from_numpy(np.frombuffer(slab, np.uint8).copy()).cuda()
            ln.copy_(_i64(sl))
            start.fill_(size)
            flen.fill_(4)
            rec_off.fill_(out_cap)
            torch.cuda.synchronize()

        # without the reserve, the framer would grow its scratch inside the capture
        g0 = torch.cuda.CUDAGraph()
        err = None
        with torch.cuda.graph(g0, stream=s):
            try:
                c.frame_fragment_streams(wire, off, ln, NCONN, start, flen, None, cap, rows, fres)
            except R.CodecError as e:
                err = str(e)
        assert err is not None and "rc=-5" in err, err
        c.reserve(cap)
        refresh(lists[0][0], lists[0][2])
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            work()                                   # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            work()
        torch.cuda.synchronize()
        for (slab, so, sl, want), srv in zip(lists[1:], servers[1:]):
            off.copy_(_i64(so))
            refresh(slab, sl)
            g.replay()
            torch.cuda.synchronize()
            n = int(want.result[0])
            assert 0 < n < cap
            assert np.array_equal(fres.cpu().numpy().view(np.uint64), want.result)
            assert np.array_equal(rows.cpu().numpy().view(np.uint64).reshape(-1, 8), want.rows)
            assert np.array_equal(start.cpu().numpy().view(np.uint64)[:n], want.frag_start)
            assert np.array_equal(flen.cpu().numpy().view(np.uint32)[:n], want.frag_len)
            assert (start.cpu().numpy()[n:cap] == size).all()
            recs = [x for c_ in range(NCONN) for x in srv.orig[c_]]
            exp, w, o = _oracle_decode(oracle, recs, L.DECODE_SLICE)
            nr = len(recs)
            r6 = dres.cpu().numpy().view(np.uint64)
            assert r6[[0, 1, 2, 3]].tolist() == [nr, n, len(w), cap - n]
            assert np.array_equal(rec_off.cpu().numpy().view(np.uint64)[:nr + 1], o)
            assert out.cpu().numpy()[:len(w)].tobytes() == w
            got = tuple(a[:2 * nr] if i == 1 else a[:nr] for i, a in enumerate(d.to_host()))
            assert_decoded_equal(got, exp, "replayed frame + defragment + decode")
    finally:
        c.close()


# ---------------------------------------------------------------------------
# 9. the C++ mirror
# ---------------------------------------------------------------------------
def _fnv1a(b):
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


def test_cpp_mirror_fragment_streams(oracle, server, tmp_path):
    """reassemble_streams and BatchDecoder::try_from_mixed_streams
    (tests/cpp_fragment_streams/test_fragment_streams.cpp) on the mixed server's
    slab."""
    exe = os.path.join(ROOT, "tests", "cpp_fragment_streams", "test_fragment_streams")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    slab, off, ln = server.slab, server.off, server.len
    src, dst = str(tmp_path / "slab.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<QQ", len(off), len(slab)) + off.tobytes() + ln.tobytes() + slab)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and "PASS test_fragment_streams" in r.stdout, r.stdout + r.stderr
    out = open(dst, "rb").read()
    # reassemble_streams of every segment
    want = FS.frame_fragment_streams(slab, off, ln)
    dm = FS.defragment_extents(slab, want.frag_start, want.frag_len)
    n_rec, n_frags, n_multi, n_bytes = struct.unpack_from("<QQQQ", out)
    assert [n_rec, n_frags, n_bytes, n_multi] == [int(want.result[2]), int(want.result[0]), int(dm["result"][2]),
                                                  int(dm["result"][5])]
    p = 32
    rows = np.frombuffer(out, np.uint64, 6 * NCONN, p).reshape(NCONN, 6)
    assert np.array_equal(rows, want.rows[:, [6, 7, 2, 3, 4, 5]])
    p += 48 * NCONN
    assert np.array_equal(np.frombuffer(out, np.uint64, n_rec + 1, p), dm["rec_off"])
    p += 8 * (n_rec + 1)
    assert not np.frombuffer(out, np.int32, n_rec, p).any()
    p += 4 * n_rec
    assert out[p:p + n_bytes] == b"".join(dm["records"]) == b"".join(x for c in range(NCONN) for x in server.orig[c])
    p += n_bytes
    # the mixed flow: one result list per connection = the oracle's decode of its original records
    rec_t = np.dtype([("st", "<i4"), ("xid", "<u4"), ("plen", "<u4"), ("fnv", "<u4")])
    for c in range(NCONN):
        n, consumed, st = struct.unpack_from("<QQQ", out, p)
        p += 24
        assert n == len(server.orig[c]) and consumed == server.whole_len[c], c
        assert st == int(want.rows[c, 3]), c
        got = np.frombuffer(out, rec_t, n, p)
        p += 16 * n
        if n == 0:
            continue
        (om, _, ost, _, _), w, _ = _oracle_decode(oracle, server.orig[c], L.DECODE_SLICE)
        assert np.array_equal(got["st"], ost), c
        ok = ost == 0
        assert np.array_equal(got["xid"][ok], om["xid"][ok]) and np.array_equal(got["plen"][ok], om["payload_len"][ok])
        fnv = [_fnv1a(w[int(a):int(a) + int(b)]) for a, b in zip(om["payload_off"][ok], om["payload_len"][ok])]
        assert got["fnv"][ok].tolist() == fnv, c
    assert p == len(out)
