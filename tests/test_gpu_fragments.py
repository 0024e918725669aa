"""Multi-fragment record streams on the device: onc_frame_fragments (the
framer's fragment mode, frame.hip) and onc_defragment (defrag.hip), every
output compared with the host model (tests/fragment_model.py) and the
oracle's encoder. tests/test_fragment_model.py proves on the CPU that each
built stream has the property its test names.

`out` is always pre-filled with a sentinel, has 64 guard bytes on each side
and starts at an odd address; rec_off and status are pre-filled too, so an
entry written past n_records shows."""
import os
import subprocess

import numpy as np
import pytest

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
    """Codecs by (frame_chunk, force_scan, variant bits), made once."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    made = {}

    def get(chunk=None, force_scan=False, variant=0):
        key = (chunk, force_scan, variant)
        if key not in made:
            made[key] = R.Codec(0, frame_chunk=chunk or 0, force_scan=force_scan, variant=variant)
        return made[key]

    yield get
    for c in made.values():
        c.close()


def _frame(R, codec, buf, max_frags=None):
    """onc_frame_fragments(buf) == the model's loop, all six outputs."""
    g = R.frame_host_fragments(codec, buf, max_frags)
    m = M.frame_fragments(buf, max_frags)
    assert g[1:] == m[1:], (g[1:], m[1:])
    assert g[0].shape == m[0].shape
    bad = np.nonzero(g[0] != m[0])[0]
    assert len(bad) == 0, f"frag_off differs first at fragment {bad[0]}: {g[0][bad[:4]]} vs {m[0][bad[:4]]}"
    return m


def _defrag(R, codec, buf, frag_off=None, out_cap=None, shift=1, wire_shift=0):
    """onc_defragment of buf's fragments (the model's offsets unless given)
    == the model: bytes (sentinel intact outside OK records, guards included),
    rec_off, status, result, unwritten tails. Returns (model, out bytes)."""
    import torch
    fo = M.frame_fragments(buf)[0] if frag_off is None else np.asarray(frag_off, np.uint64)
    nfrag = len(fo) - 1
    m = M.defragment(buf, fo, out_cap)
    need = int(m["rec_off"][-1])
    cap = need if out_cap is None else out_cap
    w = R.to_device(np.frombuffer(b"\0" * wire_shift + bytes(buf) + b"\0" * 16, np.uint8), "cuda")
    wire = w[wire_shift:]
    d_fo = torch.from_numpy(fo.view(np.int64).copy()).cuda()
    span = max(cap, need)
    base = torch.full((GUARD + 16 + span + GUARD + 16,), SENT, dtype=torch.uint8, device="cuda")
    lo = GUARD + shift
    assert (base.data_ptr() + lo) % 2 == 1 or shift != 1
    rec_off = torch.full((nfrag + 2,), -2, dtype=torch.int64, device="cuda")
    status = torch.full((nfrag + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    res = torch.full((6,), -1, dtype=torch.int64, device="cuda")
    codec.defragment(wire, d_fo, nfrag, base.data_ptr() + lo, rec_off, status, res, out_cap=cap)
    codec.sync()
    n = int(m["result"][0])
    r = res.cpu().numpy().view(np.uint64)
    assert r.tolist() == m["result"].tolist(), (r.tolist(), m["result"].tolist())
    ro = rec_off.cpu().numpy()
    assert np.array_equal(ro[:n + 1].view(np.uint64), m["rec_off"])
    assert (ro[n + 1:] == -2).all(), "rec_off written past n_records"
    st = status.cpu().numpy()
    assert st[:n].tolist() == m["status"].tolist()
    assert (st[n:] == 0x5A5A5A5A).all(), "status written from n_records on"
    got = base.cpu().numpy()
    want = np.full(got.size, SENT, np.uint8)
    want[lo:lo + span] = M.expected_out(m, span, SENT)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (f"out differs first at byte {bad[0] - lo} of {need} (cap {cap}): "
                           f"{got[bad[:8]]} vs {want[bad[:8]]}")
    return m, got[lo:lo + need].tobytes()


# ---------------------------------------------------------------------------
# 1. framer parity with onc_frame_stream
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("force_scan", [False, True])
@pytest.mark.parametrize("chunk", [None, 64, 100])
def test_framer_parity_with_record_mode(codecs, R, golden, chunk, force_scan):
    c = codecs(chunk, force_scan)
    wire, off = M.golden_stream(golden)
    for buf, mx in ((wire, None), (wire[:-3], None), (wire, 11), (wire, len(off) - 1), (b"", None), (wire, 0)):
        g = R.frame_host_fragments(c, buf, mx)
        s = R.frame_host_stream(c, buf, mx)
        assert g[1:] == s[1:] and np.array_equal(g[0], s[0]), (g[1:], s[1:])
        _frame(R, c, buf, mx)
    # the last bit cleared on chosen marks: the same offsets again
    n = len(off) - 1
    for which in ([0], [n - 1], range(1, n, 3), range(n)):
        cleared = M.clear_last_bits(wire, off, which)
        m = _frame(R, c, cleared)
        assert np.array_equal(m[0], off) and m[3] == M.OK
        assert R.frame_host_stream(c, cleared)[3] == M.FRAGMENTED


# ---------------------------------------------------------------------------
# 2. framer edges, frame_chunk = 64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("span", [0, 1, 5])
def test_continuation_fragments_spanning_chunks(codecs, R, span):
    buf = M.continuation_stream(span)
    m = _frame(R, codecs(M.EDGE_CHUNK), buf)
    assert m[2:4] == (len(buf), M.OK)
    _frame(R, codecs(M.EDGE_CHUNK, True), buf)


def test_chunks_with_only_continuation_starts(codecs, R):
    buf = M.continuation_only_stream()
    assert _frame(R, codecs(M.EDGE_CHUNK), buf)[2:4] == (len(buf), M.OK)
    _frame(R, codecs(100), buf)


@pytest.mark.parametrize("chunk", [M.EDGE_CHUNK, 1024])
def test_more_than_64_fragment_starts(codecs, R, chunk):
    """4-byte empty fragments: more starts than a chain keeps (in one chunk
    at 1024; along one chain running through unguessed chunks at 64)."""
    buf = M.empty_fragments_stream()
    for fs in (False, True):
        m = _frame(R, codecs(chunk, fs), buf)
        assert m[2:4] == (len(buf), M.OK)
        for mx in (63, 64, 65, 66, 200, m[1] - 1):
            _frame(R, codecs(chunk, fs), buf, mx)


def test_mark_straddling_a_chunk_boundary(codecs, R):
    buf = M.straddle_stream()
    c = codecs(M.EDGE_CHUNK)
    m = _frame(R, c, buf)
    assert m[2:4] == (len(buf), M.OK)
    # cut inside a straddling continuation mark, and inside its body
    fo = m[0].astype(np.int64)
    for p in fo[:-1][(fo[:-1] % M.EDGE_CHUNK >= M.EDGE_CHUNK - 3) | (fo[:-1] % M.EDGE_CHUNK <= 1)]:
        for cut in (int(p) + 1, int(p) + 3, int(p) + 4, int(p) + 6):
            _frame(R, c, buf[:cut])


def test_payload_bytes_that_look_like_headers(codecs, R):
    buf = M.header_lookalike_stream()
    for c in (codecs(M.EDGE_CHUNK), codecs(M.EDGE_CHUNK, True), codecs(100)):
        assert _frame(R, c, buf)[2:4] == (len(buf), M.OK)


def test_truncation_and_max_frags(codecs, R):
    c = codecs(M.EDGE_CHUNK)
    buf = M.continuation_stream(1)
    fo, n = M.frame_fragments(buf)[:2]
    fo = fo.astype(np.int64)
    j = n // 2
    m = _frame(R, c, buf[:fo[j] + 2])                        # mid-mark
    assert m[1:4] == (j, int(fo[j]), M.INCOMPLETE_HEADER)
    big = int(np.argmax(np.diff(fo)))                        # mid-body of the longest fragment
    cut = int(fo[big]) + 4 + 50
    m = _frame(R, c, buf[:cut])
    assert m[1:] == (big, int(fo[big]), M.INCOMPLETE_MESSAGE, cut - int(fo[big]), int(fo[big + 1] - fo[big]))
    for mx in (n - 1, n, n + 1, 0, 1):
        m = _frame(R, c, buf, mx)
        assert m[1] == min(n, mx) and m[3] == M.OK
    for tiny in FM.tiny_buffers():
        for mx in (None, 1):
            _frame(R, c, tiny, mx)
            _frame(R, codecs(), tiny, mx)


# ---------------------------------------------------------------------------
# 3. the default chunk
# ---------------------------------------------------------------------------
def test_default_chunk_with_256k_continuation_fragments(codecs, R):
    buf = M.big_continuation_stream()
    m = _frame(R, codecs(), buf)
    assert m[2:4] == (len(buf), M.OK)
    _frame(R, codecs(None, True), buf[:-7])


# ---------------------------------------------------------------------------
# 4. copy alignments
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shift", range(16))
def test_copy_every_source_and_destination_alignment(codecs, R, shift):
    """Two-fragment records with body lengths from {0, 1, 3, 15, 16, 17, 33}:
    over the 16 shifts of `out` every (source mod 16) x (destination mod 16)
    occurs (tests/test_fragment_model.py test_alignment_coverage)."""
    _defrag(R, codecs(), M.alignment_stream(), shift=shift)


# ---------------------------------------------------------------------------
# 5. copy shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", M.SHAPES)
def test_copy_shapes(codecs, R, which):
    buf = M.shapes_stream(which)
    m, _ = _defrag(R, codecs(), buf)
    assert not m["status"].any() and int(m["result"][3]) == 0
    _defrag(R, codecs(), buf, shift=16, wire_shift=3)


@pytest.mark.parametrize("kind", ["search", "slide", "spill"])
def test_copy_fragments_piled_up_at_a_tile_boundary(codecs, R, kind):
    """More fragments than the copy's staged window holds, before and at an
    output tile's first byte (`out` 1, 0 and 15 bytes past an aligned
    address). The streams are three tiles long, and the grid has a wave per
    tile: tile 1 finds its first fragment by the search in global memory,
    behind all the empty ones, and 'spill' copies it from there. The copy's
    own ways of getting there from the tile before — searching on from the
    window's end, sliding the window — are reached only when a wave runs
    several tiles: tests/test_gpu_tile_runs.py."""
    for shift in (1, 16, 15):
        _defrag(R, codecs(), M.tile_boundary_stream(kind, (GUARD + shift) % 16), shift=shift)


def test_copy_of_many_tiles_in_one_workgroup(codecs, R, originals):
    """The streams of this file that write more than four tiles, with the copy
    launched as one workgroup (ONC_VARIANT_COPY_ONE_GROUP): every wave runs
    several tiles. The same bytes as the default launch."""
    one = codecs(variant=R.VARIANT_COPY_ONE_GROUP)
    buf = M.shapes_stream("huge")
    for shift, wire_shift in ((1, 0), (16, 3)):
        assert _defrag(R, one, buf, shift=shift, wire_shift=wire_shift)[1] == _defrag(R, codecs(), buf, shift=shift)[1]
    for name, wire, off, _ in originals:
        frag = M.refragment(wire, off, M.random_cuts(1))
        m, got = _defrag(R, one, frag)
        assert got == wire and np.array_equal(m["rec_off"], off), name
        if name == "synth":
            assert len(wire) > 64 * M.TILE
            end = int(off[len(off) // 2])
            _defrag(R, one, frag, out_cap=end + 3)          # cut in the middle of the batch


# ---------------------------------------------------------------------------
# 6. pending fragments and capacity
# ---------------------------------------------------------------------------
def test_pending_fragments_and_capacity(codecs, R):
    buf, head = M.pending_stream()
    c = codecs()
    m, _ = _defrag(R, c, buf)
    assert m["result"].tolist() == [3, head, int(m["rec_off"][3]), 3, 90, 1]
    for r in (1, 2, 3):
        end = int(m["rec_off"][r])
        for cap in (end - 1, end):
            mc, _ = _defrag(R, c, buf, out_cap=cap)
            assert mc["status"].tolist() == [0 if int(e) <= cap else M.ENC_WRITE_ZERO for e in m["rec_off"][1:]]
    mc, _ = _defrag(R, c, buf, out_cap=0)
    assert mc["status"].tolist() == [M.ENC_WRITE_ZERO] * 3
    # only pending fragments; nothing at all
    tail = buf[head:]
    m, _ = _defrag(R, c, tail)
    assert m["result"].tolist() == [0, 0, 0, 3, 90, 0]
    _defrag(R, c, b"")


# ---------------------------------------------------------------------------
# 7. end to end
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def originals(oracle, golden):
    """(name, wire, rec_off, the oracle's decode of it per mode), computed once."""
    out = []
    gw, go = M.golden_stream(golden)
    sw, so, st, _ = oracle.encode_batch(S.mixed(2000, seed=77, pmin=0, pmax=900, exotic=0.2))
    assert not st.any()
    for name, w, o in (("golden", gw, go), ("synth", sw, np.asarray(so, np.uint64))):
        wa = np.frombuffer(w + b"\0" * 16, np.uint8).copy()
        out.append((name, w, o, {mode: oracle.decode_batch(wa, o, mode) for mode in MODES}))
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_end_to_end_refragmented_streams(codecs, R, originals, seed):
    c = codecs()
    for name, wire, off, decoded in originals:
        frag = M.refragment(wire, off, M.random_cuts(seed))
        fm = _frame(R, c, frag)
        assert fm[2:4] == (len(frag), M.OK)
        m, got = _defrag(R, c, frag, fm[0])
        assert got == wire and np.array_equal(m["rec_off"], off), name
        w = np.frombuffer(got + b"\0" * 16, np.uint8).copy()
        for mode in MODES:
            g = R.decode_host_wire(c, w, m["rec_off"], mode)
            assert_decoded_equal(g, decoded[mode], f"{name} mode {mode}")
        # the convenience path: framing + reassembly on the device from host bytes
        rb, ro, rs, rr, rf = R.reassemble_host_stream(c, frag)
        assert rb == wire and np.array_equal(ro, off) and not rs.any()
        assert rr.tolist() == m["result"].tolist() and rf == fm[1:]


# ---------------------------------------------------------------------------
# 8. the C++ mirror
# ---------------------------------------------------------------------------
def test_cpp_mirror_reassemble_stream(golden, tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp_defrag", "test_reassemble")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    wire, off = M.golden_stream(golden)
    frag = M.refragment(wire, off, M.random_cuts(5))
    assert FM.true_starts(frag)[2] == FM.FRAGMENTED
    pend, head = M.pending_stream()
    for tail in (b"", pend[head:]):
        (tmp_path / "orig.bin").write_bytes(wire)
        (tmp_path / "frag.bin").write_bytes(frag + tail)
        r = subprocess.run([exe, str(tmp_path / "orig.bin"), str(tmp_path / "frag.bin"), str(len(tail))],
                           capture_output=True, text=True, timeout=120)
        print(r.stdout, r.stderr)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "PASS test_reassemble" in r.stdout
