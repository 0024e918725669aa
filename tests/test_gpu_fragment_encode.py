"""Records cut into fragments on the device: onc_fragment (fragment.hip),
every output compared with the host model (tests/fragment_encode_model.py),
and through the receive side (onc_frame_fragments, onc_defragment,
onc_decode) with the oracle. tests/test_fragment_encode_model.py proves on
the CPU that each built stream has the property its test names.

`out` is always pre-filled with a sentinel, has 64 guard bytes on each side
and starts at an odd address (unless a shift says otherwise); out_off, status
and result are pre-filled too, so an entry written past its end shows."""
import os
import subprocess

import numpy as np
import pytest

import fragment_encode_model as E
import fragment_model as M
import frame_model as FM
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


def _frag(R, codec, wire, rec_off, max_frag, out_cap=None, shift=1, wire_shift=0):
    """onc_fragment of the records == the model: bytes (sentinel intact
    outside OK records, guards included), out_off, status, result. `out`
    starts GUARD + shift bytes into a 16-byte aligned buffer. Returns
    (model, the bytes the batch needs from out on)."""
    import torch
    ro = np.asarray(rec_off, np.uint64)
    n = len(ro) - 1
    m = E.fragment(wire, ro, max_frag, out_cap)
    need = int(m["out_off"][-1])
    cap = need if out_cap is None else out_cap
    w = R.to_device(np.frombuffer(b"\0" * wire_shift + bytes(wire) + b"\0" * 16, np.uint8), "cuda")
    d_ro = torch.from_numpy(ro.view(np.int64).copy()).cuda()
    span = max(cap, need)
    base = torch.full((GUARD + 16 + span + GUARD + 16,), SENT, dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 16 == 0
    lo = GUARD + shift
    out_off = torch.full((n + 2,), -2, dtype=torch.int64, device="cuda")
    status = torch.full((n + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    codec.fragment(w[wire_shift:], d_ro, n, max_frag, base.data_ptr() + lo, out_off, status, res, out_cap=cap)
    codec.sync()
    r = res.cpu().numpy()
    assert r[:3].view(np.uint64).tolist() == m["result"].tolist(), (r.tolist(), m["result"].tolist())
    assert r[3] == -1, "result written past its three words"
    oo = out_off.cpu().numpy()
    assert np.array_equal(oo[:n + 1].view(np.uint64), m["out_off"])
    assert oo[n + 1] == -2, "out_off written past n + 1"
    st = status.cpu().numpy()
    assert st[:n].tolist() == m["status"].tolist()
    assert st[n] == 0x5A5A5A5A, "status written past n"
    got = base.cpu().numpy()
    want = np.full(got.size, SENT, np.uint8)
    want[lo:lo + span] = E.expected_out(m, span, SENT)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"out differs first at byte {bad[0] - lo} of {need} (cap {cap}, max_frag {max_frag}): "
                           f"{got[bad[:8]]} vs {want[bad[:8]]}")
    return m, got[lo:lo + need].tobytes()


# ---------------------------------------------------------------------------
# 1. the golden stream
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("force_scan", [False, True])
@pytest.mark.parametrize("max_frag", E.GOLDEN_MAX_FRAGS)
def test_golden_stream(codecs, R, golden, max_frag, force_scan):
    wire, off = M.golden_stream(golden)
    m, got = _frag(R, codecs(force_scan), wire, off, max_frag)
    assert got == M.refragment(wire, off, M.fixed_cuts(max_frag))
    if max_frag == E.MAX_FRAG_LIMIT:
        assert got == wire and np.array_equal(m["out_off"], off)
    # the wire at another alignment, and the offsets from another base
    _frag(R, codecs(force_scan), wire, off, max_frag, wire_shift=5)
    w7, off7 = b"\xEE" * 7 + wire, off + np.uint64(7)
    m7, got7 = _frag(R, codecs(force_scan), w7, off7, max_frag)
    assert got7 == got and np.array_equal(m7["out_off"], m["out_off"])


@pytest.mark.parametrize("shift", range(16))
def test_golden_stream_every_out_alignment(codecs, R, golden, shift):
    wire, off = M.golden_stream(golden)
    for max_frag in (16, 17):
        _frag(R, codecs(), wire, off, max_frag, shift=shift)


# ---------------------------------------------------------------------------
# 2. copy alignments
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shift", range(16))
def test_copy_every_source_and_destination_alignment(codecs, R, shift):
    """Over the four max_frag values and the 16 shifts of `out` the chunks
    moved 16 bytes at a time cover every (source mod 16) x (destination mod
    16) (tests/test_fragment_encode_model.py asserts the coverage)."""
    wire, off = E.alignment_stream()
    for max_frag in E.ALIGN_MAX_FRAGS:
        _frag(R, codecs(), wire, off, max_frag, shift=shift)


# ---------------------------------------------------------------------------
# 3. fragment-count edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("F", E.COUNT_EDGE_FS)
def test_fragment_count_edges(codecs, R, F):
    wire, off = E.count_edges_stream(F)
    m, got = _frag(R, codecs(), wire, off, F)
    assert got == M.refragment(wire, off, M.fixed_cuts(F))
    _frag(R, codecs(), wire, off, F, shift=16, wire_shift=3)


# ---------------------------------------------------------------------------
# 4. many records per tile
# ---------------------------------------------------------------------------
def test_more_records_in_a_tile_than_the_staged_window(codecs, R):
    wire, off = E.empty_records_stream()
    for max_frag, shift in ((8, 1), (100, 16)):
        m, _ = _frag(R, codecs(), wire, off, max_frag, shift=shift)
        assert E.records_reaching_into_tiles(m).max() > E.STAGE
    wire, off = E.short_records_stream()
    m, _ = _frag(R, codecs(), wire, off, 8)
    assert m["result"].tolist() == [1500, 16000, 500]


# ---------------------------------------------------------------------------
# 5. one large record
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_frag", [7, 8188, 70_001, 100_000])
def test_one_large_record(codecs, R, max_frag):
    wire, off = E.large_record_stream()
    m, got = _frag(R, codecs(), wire, off, max_frag)
    assert not m["status"].any()
    _frag(R, codecs(), wire, off, max_frag, shift=16, wire_shift=3)
    # and back through the receive side
    rb, ro, rs, rr, rf = R.reassemble_host_stream(codecs(), got)
    assert rb == wire and np.array_equal(ro, off) and not rs.any() and rf[0] == int(m["result"][0])


@pytest.mark.parametrize("max_frag", [7, 8188, 70_001, 100_000])
def test_one_large_record_in_one_workgroup(codecs, R, max_frag):
    """The copy launched as one workgroup (ONC_VARIANT_COPY_ONE_GROUP): 13
    tiles and more, several per wave (tests/test_gpu_tile_runs.py). The same
    bytes as the default launch, whole and cut by the capacity."""
    wire, off = E.large_record_stream()
    one = codecs(variant=R.VARIANT_COPY_ONE_GROUP)
    for shift, wire_shift in ((1, 0), (16, 3)):
        assert _frag(R, one, wire, off, max_frag, shift=shift, wire_shift=wire_shift)[1] == \
            _frag(R, codecs(), wire, off, max_frag, shift=shift)[1]
    for cap in (50_000, 28):
        _frag(R, one, wire, off, max_frag, out_cap=cap)


# ---------------------------------------------------------------------------
# 6. tile boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [16, 1, 15])
def test_marks_and_records_at_a_tile_boundary(codecs, R, shift):
    """A synthesised mark starting 0..4 bytes before an output tile's first
    byte, and a record starting exactly there (`out` 0, 1 and 15 bytes past
    an aligned address)."""
    origin = (GUARD + shift) % 16
    F = E.TILE_MARK_FRAG
    for d in range(5):
        wire, off = E.tile_mark_stream(d, origin)
        m, _ = _frag(R, codecs(), wire, off, F, shift=shift)
        pos, cont = E.mark_positions(m, F)
        assert (E.TILE - origin - d) in pos[cont].tolist()
    wire, off = E.tile_record_boundary_stream(origin)
    m, _ = _frag(R, codecs(), wire, off, F, shift=shift)
    assert (E.TILE - origin) in m["out_off"].tolist()


# ---------------------------------------------------------------------------
# 7. extents that are no records, the empty batch, the plan's block edges
# ---------------------------------------------------------------------------
def test_non_record_extents(codecs, R):
    c = codecs()
    wire, off = E.non_record_extents("mixed")
    for max_frag in (1, 16, 1000):
        m, _ = _frag(R, c, wire, off, max_frag)
        assert set(m["status"].tolist()) == {E.OK, E.ENC_BAD_DESCRIPTOR}
    wire, off = E.non_record_extents("only")
    m, _ = _frag(R, c, wire, off, 16)
    assert m["result"].tolist() == [0, 0, 0]
    _frag(R, c, wire, off, 16, out_cap=0)
    m, _ = _frag(R, c, b"", np.zeros(1, np.uint64), 16)
    assert m["result"].tolist() == [0, 0, 0] and m["out_off"].tolist() == [0]


@pytest.mark.parametrize("n", [255, 256, 257, 1025])
def test_plan_block_edges(codecs, R, n):
    wire, off = E.short_records(n)
    for fs in (False, True):
        _frag(R, codecs(fs), wire, off, 9)


# ---------------------------------------------------------------------------
# 8. capacity
# ---------------------------------------------------------------------------
def test_capacity(codecs, R):
    c = codecs()
    wire, off = E.non_record_extents("mixed")
    full = E.fragment(wire, off, 16)
    need = int(full["out_off"][-1])
    big = int(full["out_off"][8])                   # the record of 40 body bytes: 16 + 16 + 8
    lens = np.diff(off.astype(np.int64))
    for cap in (need, need - 1, big + 4 + 16 + 4 + 6, big, 0):
        m, _ = _frag(R, c, wire, off, 16, out_cap=cap)
        assert np.array_equal(m["out_off"], full["out_off"]) and np.array_equal(m["result"], full["result"])
        ends = full["out_off"][1:].astype(np.int64)
        want = [E.ENC_BAD_DESCRIPTOR if 0 < l < 4 else E.OK if l == 0 or e <= cap else E.ENC_WRITE_ZERO
                for l, e in zip(lens, ends)]
        assert m["status"].tolist() == want
    assert lens[-1] == 0 and want[-1] == E.OK       # a zero-length extent after the first non-fitting record
    # a larger stream cut in the middle of a tile and of a fragment
    wire, off = E.large_record_stream()
    for cap in (50_000, 27, 28):
        m, _ = _frag(R, c, wire, off, 8188, out_cap=cap)
        assert m["status"].tolist() == [E.OK if cap >= 28 else E.ENC_WRITE_ZERO, E.ENC_WRITE_ZERO, E.ENC_WRITE_ZERO]


# ---------------------------------------------------------------------------
# 9. the device round trip
# ---------------------------------------------------------------------------
def test_device_round_trip(codecs, R, oracle):
    """onc_encode -> onc_fragment -> onc_frame_stream (Fragmented) ->
    onc_frame_fragments -> onc_defragment -> onc_decode, against the oracle's
    encoder and decoder."""
    c = codecs()
    hb = L.build_batch(S.random_messages(300, seed=21, max_payload=700))
    # an AuthShort verifier of 201 bytes: the reference's assert (> 200), no bytes written
    hb.msgs["verf_kind_len"][np.arange(0, hb.n, 37)] = int(L.pack_kind_len(L.KIND_SHORT, 201))
    g_wire, g_off, g_st, _ = R.encode_host_batch(c, hb)
    o_wire, o_off, o_st, _ = oracle.encode_batch(hb)
    assert g_wire == o_wire and np.array_equal(g_off, np.asarray(o_off, np.uint64)) and np.array_equal(g_st, o_st)
    lens = np.diff(g_off.astype(np.int64))
    assert (g_st != 0).sum() >= 5 and (lens[g_st != 0] == 0).all(), "failing records with empty extents"
    m, frag = _frag(R, c, g_wire, g_off, 64)
    assert int(m["result"][2]) > 0
    assert R.frame_host_stream(c, frag)[3] == M.FRAGMENTED
    rb, ro, rs, rr, rf = R.reassemble_host_stream(c, frag)
    kept = np.concatenate((g_off[:-1][lens > 0], g_off[-1:]))
    assert rb == o_wire and np.array_equal(ro, kept) and not rs.any()
    assert rf[:3] == (int(m["result"][0]), len(frag), M.OK) and int(rr[5]) == int(m["result"][2])
    w = np.frombuffer(rb + b"\0" * 16, np.uint8).copy()
    for mode in MODES:
        assert_decoded_equal(R.decode_host_wire(c, w, ro, mode), oracle.decode_batch(w, kept, mode), f"mode {mode}")
    # the convenience path gives the same bytes
    fb, fo, fs, fr = R.fragment_host(c, g_wire, g_off, 64, shift=3)
    assert fb == frag and np.array_equal(fo, m["out_off"]) and np.array_equal(fs, m["status"])
    assert fr.tolist() == m["result"].tolist()


# ---------------------------------------------------------------------------
# 10. graph capture
# ---------------------------------------------------------------------------
def test_graph_capture_and_replay(R, golden):
    import torch
    wire, off = M.golden_stream(golden)
    n = len(off) - 1
    # a second input of the same shape: the same extents, other bytes
    rng = np.random.default_rng(5)
    wire2 = rng.bytes(len(wire))
    F = 16
    m1, m2 = E.fragment(wire, off, F), E.fragment(wire2, off, F)
    need = int(m1["out_off"][-1])
    w = R.to_device(np.frombuffer(wire + b"\0" * 16, np.uint8), "cuda")
    d_ro = torch.from_numpy(off.view(np.int64).copy()).cuda()
    base = torch.full((GUARD + 16 + need + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    lo = GUARD + 1
    out_off = torch.full((n + 1,), -2, dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()

    def work(codec):
        codec.fragment(w, d_ro, n, F, base.data_ptr() + lo, out_off, status, res, out_cap=need)

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
        for wi, m in ((wire, m1), (wire2, m2)):
            w.copy_(torch.from_numpy(np.frombuffer(wi + b"\0" * 16, np.uint8).copy()))
            base.fill_(SENT)
            g.replay()
            torch.cuda.synchronize()
            got = base.cpu().numpy()
            want = np.full(got.size, SENT, np.uint8)
            want[lo:lo + need] = E.expected_out(m, need, SENT)
            assert np.array_equal(got, want)
            assert np.array_equal(out_off.cpu().numpy().view(np.uint64), m["out_off"])
            assert not status.cpu().numpy().any()
            assert res.cpu().numpy().view(np.uint64).tolist() == m["result"].tolist()
    finally:
        fresh.close()
        codec.close()


# ---------------------------------------------------------------------------
# 11. the C++ mirror
# ---------------------------------------------------------------------------
def test_cpp_mirror_fragment_stream(golden, tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp_fragment", "test_fragment")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    wire, _ = M.golden_stream(golden)
    (tmp_path / "orig.bin").write_bytes(wire)
    for max_frag in (16, 1000):
        r = subprocess.run([exe, str(tmp_path / "orig.bin"), str(max_frag)], capture_output=True, text=True,
                           timeout=120)
        print(r.stdout, r.stderr)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "PASS test_fragment" in r.stdout
