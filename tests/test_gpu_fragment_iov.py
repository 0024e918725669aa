"""The vectored encode's records cut into fragments without a copy:
onc_fragment_iov (fragment_iov.hip). Every table, piece and mark is compared
with the host model (tests/fragment_iov_model.py), the gathered bytes with
the packed path's model (fragment_encode_model.fragment) over the oracle's
encoder, and the stream goes back through the receive side.
tests/test_fragment_iov_model.py proves on the CPU that each built entry list
has the property its test names.

`marks` and `pieces` are pre-filled with a sentinel and have 64 guard bytes on
each side; out_off, piece_off, status and result are pre-filled too, so an
entry written past its end shows."""
import functools
import os
import subprocess

import numpy as np
import pytest

import fragment_encode_model as E
import fragment_iov_model as V
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
from test_gpu_parity import assert_decoded_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xA5
GUARD = 64
MODES = [L.DECODE_SLICE, L.DECODE_BYTES]


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codecs(R):
    """Codecs by (force_scan, variant bits), made once."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    made = {}

    def get(force_scan=False, variant=0):
        if (force_scan, variant) not in made:
            made[force_scan, variant] = R.Codec(0, force_scan=force_scan, variant=variant)
        return made[force_scan, variant]

    yield get
    for c in made.values():
        c.close()


def _fiv(R, codec, iov, max_frag, lim=None, max_pieces=None, marks_cap=None, d_iov=None):
    """onc_fragment_iov of the entries == the model: the written pieces and
    marks (the sentinel intact everywhere else, guards included), out_off,
    piece_off, status, result. Returns the model."""
    import torch
    n = len(iov)
    m = V.fragment_iov(iov, max_frag, lim, max_pieces, marks_cap)
    need_p, need_m = int(m["result"][3]), 4 * int(m["result"][0])
    pcap = need_p if max_pieces is None else max_pieces
    mcap = need_m if marks_cap is None else marks_cap
    if d_iov is None:
        d_iov = R.to_device(np.ascontiguousarray(iov), "cuda")
    d_lim = None
    if lim is not None:
        d_lim = torch.from_numpy(np.append(np.asarray(lim, np.uint32), np.uint32(0)).view(np.int32).copy()).cuda()
    pspan, mspan = 16 * max(pcap, need_p), (max(mcap, need_m) + 3) // 4 * 4
    pbuf = torch.full((GUARD + pspan + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    mbuf = torch.full((GUARD + mspan + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    assert pbuf.data_ptr() % 16 == 0 and mbuf.data_ptr() % 16 == 0
    out_off = torch.full((n + 2,), -2, dtype=torch.int64, device="cuda")
    piece_off = torch.full((n + 2,), -3, dtype=torch.int64, device="cuda")
    status = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    res = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    codec.fragment_iov(d_iov, n, max_frag, mbuf.data_ptr() + GUARD, pbuf.data_ptr() + GUARD, out_off, piece_off,
                       status, res, rec_max_frag=d_lim, marks_cap=mcap, max_pieces=pcap)
    codec.sync()
    r = res.cpu().numpy()
    assert r[:4].view(np.uint64).tolist() == m["result"].tolist(), (r.tolist(), m["result"].tolist())
    assert r[4] == -1, "result written past its four words"
    oo, po = out_off.cpu().numpy(), piece_off.cpu().numpy()
    assert np.array_equal(oo[:n + 1].view(np.uint64), m["out_off"]) and oo[n + 1] == -2
    assert np.array_equal(po[:n + 1].view(np.uint64), m["piece_off"]) and po[n + 1] == -3
    st = status.cpu().numpy()
    assert st[:n].tolist() == m["status"].tolist()
    assert st[n] == 0x5A5A5A5A, "status written past n"
    w = len(m["pieces"])
    assert w <= pcap and len(m["marks"]) <= mcap
    got_p = pbuf.cpu().numpy()
    want_p = np.full(got_p.size, SENT, np.uint8)
    want_p[GUARD:GUARD + 16 * w] = m["pieces"].view(np.uint8)
    bad = np.nonzero(got_p != want_p)[0]
    assert len(bad) == 0, (f"pieces differ first at piece {(bad[0] - GUARD) // 16} of {w} (capacity {pcap}, max_frag "
                           f"{max_frag}): {got_p[bad[:8]]} vs {want_p[bad[:8]]}")
    got_m = mbuf.cpu().numpy()
    want_m = np.full(got_m.size, SENT, np.uint8)
    want_m[GUARD:GUARD + len(m["marks"])] = np.frombuffer(m["marks"], np.uint8)
    bad = np.nonzero(got_m != want_m)[0]
    assert len(bad) == 0, (f"marks differ first at byte {bad[0] - GUARD} of {len(m['marks'])} (capacity {mcap}, "
                           f"max_frag {max_frag})")
    return m


def _encode_iov(R, codec, hb):
    """onc_encode_iov of a host batch -> (hdr bytes, iov, status, the device
    entries)."""
    import torch
    db = R.DeviceBatch.from_host(hb, "cuda")
    n = hb.n
    cap = int(R.codec_lengths(codec, db).sum())
    hdr = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    d_iov = torch.zeros(max(1, n) * 32, dtype=torch.uint8, device="cuda")
    st = torch.full((max(1, n),), -1, dtype=torch.int32, device="cuda")
    codec.encode_iov(db, hdr, d_iov, st, None, hdr_cap=cap)
    codec.sync()
    return hdr.cpu().numpy(), d_iov.cpu().numpy().view(L.IOV_DTYPE)[:n].copy(), st.cpu().numpy()[:n].copy(), d_iov, st


# ---------------------------------------------------------------------------
# 1. parity with the packed path
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed(n):
    return S.mixed(n, seed=300 + n % 89, pmin=0, pmax=300, exotic=0.2)


@pytest.mark.parametrize("force_scan", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_parity_with_the_packed_path(codecs, R, oracle, n, force_scan):
    hb = _mixed(n)
    c = codecs(force_scan)
    o_wire, o_off, o_st, _ = oracle.encode_batch(hb)
    o_off = np.asarray(o_off, np.uint64)
    hdr, iov, st, d_iov, _ = _encode_iov(R, c, hb)
    assert np.array_equal(st, o_st)
    for max_frag in E.GOLDEN_MAX_FRAGS:
        if max_frag == 1 and n > 257:
            continue
        m = _fiv(R, c, iov, max_frag, d_iov=d_iov)
        p = E.fragment(o_wire, o_off, max_frag)
        got = V.gather(m["pieces"], m["marks"], hdr, hb.payload_arena)
        assert got == E.stream_bytes(p), f"n {n} max_frag {max_frag}"
        if max_frag == E.MAX_FRAG_LIMIT:
            assert got == bytes(o_wire)
        assert np.array_equal(m["out_off"], p["out_off"]) and np.array_equal(m["status"], p["status"])
        assert m["result"][:3].tolist() == p["result"].tolist()


# ---------------------------------------------------------------------------
# 2. the header / payload boundary
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("F", V.BOUNDARY_FS)
def test_header_payload_boundary(codecs, R, F):
    iov = V.boundary_stream(F)[0]
    m = _fiv(R, codecs(), iov, F)
    assert set(m["status"].tolist()) == {V.OK, V.ENC_BAD_DESCRIPTOR}
    _fiv(R, codecs(True), iov, F)


# ---------------------------------------------------------------------------
# 3. the fill's tiles and the plan's blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("t", sorted(V.STRADDLE_KINDS))
def test_record_straddles_a_tile_boundary(codecs, R, t):
    m = _fiv(R, codecs(), V.tile_straddle_stream(t)[0], V.STRADDLE_F)
    assert int(m["pieces"]["src"][V.TILE]) == V.STRADDLE_KINDS[t]


def test_more_records_in_a_tile_than_the_staged_window(codecs, R):
    m = _fiv(R, codecs(), V.bare_marks_stream()[0], 16)
    assert V.records_reaching_into_tiles(m).max() > V.STAGE


def test_one_record_of_many_tiles(codecs, R):
    iov, hdr, pay, wire, off = V.large_record_stream()
    m = _fiv(R, codecs(), iov, 7)
    assert int(np.diff(m["piece_off"].astype(np.int64)).max()) > 4 * V.TILE
    assert V.gather(m["pieces"], m["marks"], hdr, pay) == E.stream_bytes(E.fragment(wire, off, 7))


def test_many_tiles_in_one_workgroup(codecs, R):
    """The lists of this file that fill more than four tiles, with the fill
    launched as one workgroup (ONC_VARIANT_COPY_ONE_GROUP): several tiles per
    wave (tests/test_gpu_tile_runs.py). The same pieces and marks as the
    default launch, whole and cut by a capacity."""
    one = codecs(variant=R.VARIANT_COPY_ONE_GROUP)
    for iov, F in ((V.bare_marks_stream()[0], 16), (V.large_record_stream()[0], 7)):
        a, b = _fiv(R, one, iov, F), _fiv(R, codecs(), iov, F)
        assert len(a["pieces"]) > 4 * V.TILE and np.array_equal(a["pieces"], b["pieces"]) and a["marks"] == b["marks"]
    _fiv(R, one, V.bare_marks_stream()[0], 16, max_pieces=5 * V.TILE + 188)
    for kw in ({"max_pieces": 3 * V.TILE + 17}, {"marks_cap": 4 * 700 + 2}):
        _fiv(R, one, V.large_record_stream()[0], 7, **kw)


@pytest.mark.parametrize("n", [255, 256, 257, 1025])
def test_plan_block_edges(codecs, R, n):
    iov = V.short_records(n)[0]
    for fs in (False, True):
        _fiv(R, codecs(fs), iov, 9)


# ---------------------------------------------------------------------------
# 4. a limit per record
# ---------------------------------------------------------------------------
def test_per_record_limits(codecs, R):
    (iov, hdr, pay, wire, off), lim = V.per_record_stream()
    m = _fiv(R, codecs(), iov, 16, lim=lim)          # neighbours of invalid entries included: all equal the model
    assert (m["status"] == V.ENC_BAD_DESCRIPTOR).sum() >= 3
    # NULL is an array filled with max_frag
    u = _fiv(R, codecs(), iov, 16, lim=np.full(len(iov), 16, np.uint32))
    v = _fiv(R, codecs(), iov, 16)
    assert np.array_equal(u["pieces"], v["pieces"]) and u["marks"] == v["marks"]
    # max_frag is ignored when the array is given
    w = _fiv(R, codecs(), iov, 3, lim=np.full(len(iov), 16, np.uint32))
    assert np.array_equal(w["pieces"], v["pieces"]) and w["marks"] == v["marks"]


# ---------------------------------------------------------------------------
# 5. capacities
# ---------------------------------------------------------------------------
def test_capacities(codecs, R):
    c = codecs()
    iov = V.build(V.random_splits(60, 11), seed=11)[0]
    full = V.fragment_iov(iov, 16)
    tot_p, tot_m = int(full["result"][3]), 4 * int(full["result"][0])
    po = full["piece_off"].astype(np.int64)
    big = int(np.argmax(np.diff(po)[:-1]))           # a record of several pieces, not the last
    assert po[big + 1] - po[big] >= 4
    nf = np.concatenate(([0], np.cumsum([len(V.fragment_iov(iov[i:i + 1], 16)["marks"]) for i in range(len(iov))])))
    assert nf[-1] == tot_m and nf[big + 1] - nf[big] >= 8
    cuts = [{"max_pieces": 0}, {"max_pieces": int(po[big]) + 2}, {"max_pieces": int(po[big])},
            {"max_pieces": tot_p - 1}, {"max_pieces": tot_p},
            {"marks_cap": 0}, {"marks_cap": int(nf[big]) + 4}, {"marks_cap": int(nf[big])},
            {"marks_cap": tot_m - 1}, {"marks_cap": int(nf[big + 1]) + 3}, {"marks_cap": 3},
            {"max_pieces": int(po[big]) + 2, "marks_cap": int(nf[big]) - 4 if nf[big] >= 4 else 0},
            {"max_pieces": 0, "marks_cap": 0}]
    for kw in cuts:
        m = _fiv(R, c, iov, 16, **kw)                # sentinels beyond both capacities and after the last piece
        for k in ("out_off", "piece_off", "result"):
            assert np.array_equal(m[k], full[k]), (kw, k)
        short = kw.get("max_pieces", tot_p) < tot_p or kw.get("marks_cap", tot_m) < tot_m
        assert (V.ENC_WRITE_ZERO in m["status"].tolist()) == short, kw
    # a record of many tiles that does not fit: nothing of it is written
    iov = V.large_record_stream()[0]
    for kw in ({"max_pieces": 3 * V.TILE + 17}, {"marks_cap": 4 * 700 + 2}):
        m = _fiv(R, c, iov, 7, **kw)
        assert m["status"].tolist() == [V.OK, V.ENC_WRITE_ZERO, V.ENC_WRITE_ZERO]
    # the written pieces end in the middle of a tile
    m = _fiv(R, c, V.bare_marks_stream()[0], 16, max_pieces=V.TILE + 188)
    assert len(m["pieces"]) == V.TILE + 188
    m = _fiv(R, c, V.short_records(1025)[0], 9, marks_cap=4 * 1001 + 1)
    assert 0 < len(m["pieces"]) < int(m["result"][3]) and len(m["pieces"]) % V.TILE != 0


# ---------------------------------------------------------------------------
# 6. placeholders and failing records
# ---------------------------------------------------------------------------
def test_placeholders_and_failing_records(codecs, R, oracle):
    from test_gpu_emit_paths import _adversarial
    c = codecs()
    hb = _adversarial(75, n=2500)
    o_wire, o_off, o_st, o_len = oracle.encode_batch(hb)
    o_off = np.asarray(o_off, np.uint64)
    assert ((o_st != 0) & (o_len != 0)).any() and ((o_st != 0) & (o_len == 0)).any()
    hdr, iov, st, d_iov, d_st = _encode_iov(R, c, hb)
    assert np.array_equal(st, o_st)
    F = 64
    # uncompacted: a placeholder is a record like any other
    m = _fiv(R, c, iov, F, d_iov=d_iov)
    p = E.fragment(o_wire, o_off, F)
    assert V.gather(m["pieces"], m["marks"], hdr, hb.payload_arena) == E.stream_bytes(p)
    assert np.array_equal(m["out_off"], p["out_off"]) and m["result"][:3].tolist() == p["result"].tolist()
    # compacted: the failing records' extents dropped
    c.compact_iov(d_iov, d_st, hb.n)
    c.sync()
    iov2 = d_iov.cpu().numpy().view(L.IOV_DTYPE)[:hb.n].copy()
    lens = np.where(o_st == 0, np.diff(o_off.astype(np.int64)), 0)
    w2 = b"".join(bytes(o_wire[int(o_off[i]):int(o_off[i + 1])]) for i in np.nonzero(o_st == 0)[0])
    off2 = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    m2 = _fiv(R, c, iov2, F, d_iov=d_iov)
    p2 = E.fragment(w2, off2, F)
    assert V.gather(m2["pieces"], m2["marks"], hdr, hb.payload_arena) == E.stream_bytes(p2)
    assert np.array_equal(m2["out_off"], p2["out_off"]) and not m2["status"].any()


# ---------------------------------------------------------------------------
# 7. the round trip
# ---------------------------------------------------------------------------
def test_round_trip(codecs, R, oracle):
    """onc_encode_iov -> onc_fragment_iov -> gather on the host ->
    onc_frame_fragments -> onc_defragment -> onc_decode, against onc_encode's
    bytes and the oracle's decoder."""
    c = codecs()
    hb = L.build_batch(S.random_messages(300, seed=23, max_payload=700))
    g_wire, g_off, g_st, _ = R.encode_host_batch(c, hb)
    assert not g_st.any()
    hdr, iov, st, d_iov, _ = _encode_iov(R, c, hb)
    m = _fiv(R, c, iov, 64, d_iov=d_iov)
    assert int(m["result"][2]) > 0
    stream = V.gather(m["pieces"], m["marks"], hdr, hb.payload_arena)
    rb, ro, rs, rr, rf = R.reassemble_host_stream(c, stream)
    assert rb == g_wire and np.array_equal(ro, g_off) and not rs.any()
    assert rf[:3] == (int(m["result"][0]), len(stream), 0) and int(rr[5]) == int(m["result"][2])
    w = np.frombuffer(rb + b"\0" * 16, np.uint8).copy()
    for mode in MODES:
        assert_decoded_equal(R.decode_host_wire(c, w, ro, mode), oracle.decode_batch(w, g_off, mode), f"mode {mode}")
    # the convenience path gives the same arrays
    marks, pieces, oo, po, fs, fr = R.fragment_iov_host(c, iov, 64)
    assert np.array_equal(pieces, m["pieces"]) and marks.tobytes() == m["marks"]
    assert np.array_equal(oo, m["out_off"]) and np.array_equal(po, m["piece_off"])
    assert fr.tolist() == m["result"].tolist() and not fs.any()
    assert R.gather_pieces(pieces, marks, hdr, hb.payload_arena) == stream


# ---------------------------------------------------------------------------
# 8. graph capture
# ---------------------------------------------------------------------------
def test_graph_capture_and_replay(R):
    import torch
    iov1 = V.build(V.random_splits(300, 31), seed=31)[0]
    iov2 = V.build(V.random_splits(300, 32), seed=32)[0]
    n, F = 300, 16
    m1, m2 = V.fragment_iov(iov1, F), V.fragment_iov(iov2, F)
    pcap = max(int(m1["result"][3]), int(m2["result"][3]))
    mcap = 4 * max(int(m1["result"][0]), int(m2["result"][0]))
    d_iov = R.to_device(iov1, "cuda")
    pbuf = torch.full((16 * pcap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    mbuf = torch.full((mcap + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    out_off = torch.full((n + 1,), -2, dtype=torch.int64, device="cuda")
    piece_off = torch.full((n + 1,), -2, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def work(codec):
        codec.fragment_iov(d_iov, n, F, mbuf, pbuf, out_off, piece_off, status, res, marks_cap=mcap, max_pieces=pcap)

    fresh = R.Codec(0, stream=s.cuda_stream)
    codec = R.Codec(0, stream=s.cuda_stream)
    try:
        err = None
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            try:
                work(fresh)
            except R.CodecError as e:
                err = str(e)
        assert err is not None and "rc=-5" in err, err
        codec.reserve(n)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            work(codec)                              # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            work(codec)
        torch.cuda.synchronize()
        for e, m in ((iov1, m1), (iov2, m2)):
            d_iov.copy_(torch.from_numpy(e.view(np.uint8).copy()))
            pbuf.fill_(SENT)
            mbuf.fill_(SENT)
            g.replay()
            torch.cuda.synchronize()
            w = len(m["pieces"])
            got_p, got_m = pbuf.cpu().numpy(), mbuf.cpu().numpy()
            assert np.array_equal(got_p[:16 * w].view(V.PIECE_DTYPE), m["pieces"]) and (got_p[16 * w:] == SENT).all()
            assert got_m[:len(m["marks"])].tobytes() == m["marks"] and (got_m[len(m["marks"]):] == SENT).all()
            assert np.array_equal(out_off.cpu().numpy().view(np.uint64), m["out_off"])
            assert np.array_equal(piece_off.cpu().numpy().view(np.uint64), m["piece_off"])
            assert status.cpu().numpy().tolist() == m["status"].tolist()
            assert res.cpu().numpy().view(np.uint64).tolist() == m["result"].tolist()
    finally:
        fresh.close()
        codec.close()


# ---------------------------------------------------------------------------
# 9. the C++ mirror
# ---------------------------------------------------------------------------
def test_cpp_mirror_serialise_vectored():
    exe = os.path.join(ROOT, "tests", "cpp_fragment_iov", "test_fragment_iov")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_fragment_iov" in r.stdout
