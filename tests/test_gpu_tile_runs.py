"""The copy kernels' runs of tiles on the device, at sizes a test can afford.

defrag_copy, frag_copy, gather_copy, place_copy and fragiov_fill deal their
output tiles out among the waves of the grid; a wave that gets more than one
carries its place in the sorted positions from tile to tile (walk_tiles in
onc-rpc_amd/csrc/tile_walk.h; tests/tile_walk_model.py restates that walk). The default grid has a wave per
tile up to 64 MiB of output, so every other test of these kernels runs tiles
that search for themselves. A codec made with ONC_VARIANT_COPY_ONE_GROUP
launches the same kernels as one workgroup: 5 to 13 tiles then make runs of 2
to 4 per wave. tests/test_tile_walk_model.py proves on the CPU that each case
here takes the outcome it is named for — research, slide, global, a long entry
under which ja stays, a capacity cut — on a tile that is not the first of its
run in one workgroup, and on none at the default grid.

Every case runs through the real entry points on both codecs and is compared
bit-exactly with the host models by the sibling files' own checkers (sentinel
fill, guard bands, unwritten tails); where a checker returns the output, the
two codecs' outputs are compared byte for byte as well. heads_gather's
grid-stride loop is in the same position and is run here with four steps."""
import numpy as np
import pytest

import fragment_encode_model as E
import fragment_iov_model as V
import fragment_model as M
import fragment_streams_model as FS
import gather_model as G
import heads_model as HM
import payload_model as PM
import test_gpu_fragment_encode as TE
import test_gpu_fragment_iov as TV
import test_gpu_fragment_streams as TS
import test_gpu_fragments as TF
import test_gpu_gather as TG
import test_gpu_payload as TP
import test_tile_walk_model as TM
import tile_walk_model as TW

pytestmark = pytest.mark.gpu

SENT = 0xA5
U64, U32 = np.uint64(2**64 - 1), 0xFFFFFFFF
CASES, CUTS = TM.CASES, TM.CUTS


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def pair(R):
    """(the default codec, one that launches the copy kernels as one workgroup)."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    cs = (R.Codec(0), R.Codec(0, variant=R.VARIANT_COPY_ONE_GROUP))
    yield cs
    for c in cs:
        c.close()


def _both(pair, run):
    """run(codec) on both codecs; what it returns must be the same bytes."""
    a, b = run(pair[0]), run(pair[1])
    assert a == b, "the one-workgroup launch and the default one disagree"
    return b


# ---------------------------------------------------------------------------
# onc_defragment, onc_defragment_extents
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ntiles,origin", CASES)
def test_defragment(R, pair, kind, ntiles, origin):
    buf, _ = M.tile_run_stream(kind, ntiles, origin)
    _both(pair, lambda c: TF._defrag(R, c, buf, shift=origin)[1])


@pytest.mark.parametrize("kind,ntiles,origin", CASES)
def test_defragment_extents(R, pair, kind, ntiles, origin):
    buf, _ = M.tile_run_stream(kind, ntiles, origin)
    wire, start, flen = FS.scatter(buf, "shuffled", seed=ntiles + origin)
    got = _both(pair, lambda c: TS._defrag_ext(R, c, wire, start, flen, shift=origin)[1])
    assert got == b"".join(M.defragment(buf, M.frame_fragments(buf)[0])["records"])


@pytest.mark.parametrize("origin", TW.ORIGINS)
@pytest.mark.parametrize("ntiles", CUTS)
def test_defragment_capacity_cut(R, pair, ntiles, origin):
    """The capacity ends inside the last tile written; nothing past the last
    record that fits is written (the checker compares the whole capacity, the
    needed bytes beyond it and the guards with the sentinel)."""
    buf, cap, W = TM.defragment_cut(ntiles, origin)
    for c in pair:
        m, _ = TF._defrag(R, c, buf, out_cap=cap, shift=origin)
        st = m["status"].tolist()
        assert st.count(M.OK) > 0 and st == sorted(st) and st[-1] == M.ENC_WRITE_ZERO
        assert int(m["rec_off"][st.count(M.OK)]) == W
    wire, start, flen = FS.scatter(buf, "descending")
    for c in pair:
        TS._defrag_ext(R, c, wire, start, flen, out_cap=cap, shift=origin)


# ---------------------------------------------------------------------------
# onc_fragment
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ntiles,origin", CASES)
def test_fragment(R, pair, kind, ntiles, origin):
    wire, off = E.tile_run_stream(kind, ntiles, origin)
    got = _both(pair, lambda c: TE._frag(R, c, wire, off, E.TILE_RUN_FRAG, shift=origin)[1])
    recs = [wire[int(a):int(b)] for a, b in zip(off[:-1], off[1:]) if b - a >= 4]      # the extents that are records
    assert got == M.refragment(b"".join(recs), E.offsets_of(recs), M.fixed_cuts(E.TILE_RUN_FRAG))


@pytest.mark.parametrize("origin", TW.ORIGINS)
@pytest.mark.parametrize("ntiles", CUTS)
def test_fragment_capacity_cut(R, pair, ntiles, origin):
    wire, off, cap, W = TM.fragment_cut(ntiles, origin)
    for c in pair:
        m, _ = TE._frag(R, c, wire, off, E.TILE_RUN_FRAG, out_cap=cap, shift=origin)
        assert E.ENC_WRITE_ZERO in m["status"].tolist()


# ---------------------------------------------------------------------------
# onc_piece_offsets + onc_gather_pieces
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ntiles,origin", CASES)
def test_gather(R, pair, kind, ntiles, origin):
    pieces, sources = G.tile_run_list(kind, ntiles, origin)
    outs = []
    for c in pair:
        lst = TG.Listed(R, c, pieces, sources)
        assert int(lst.res[1]) == 0
        outs.append(lst.window(0, lst.total, origin).tobytes())
    assert outs[0] == outs[1] == G.stream(pieces, sources).tobytes()


@pytest.mark.parametrize("origin", TW.ORIGINS)
@pytest.mark.parametrize("ntiles", TW.SIZES)
def test_gather_windows(R, pair, ntiles, origin):
    """Windows that start and end inside carried tiles and in the run of empty
    pieces, and run past the stream's end (tests/test_tile_walk_model.py
    test_gather_windows says what they reach)."""
    pieces, sources = G.tile_run_list("research", ntiles, origin)
    windows = TM.gather_windows(ntiles, origin)[0]
    lists = [TG.Listed(R, c, pieces, sources) for c in pair]
    for start, count in windows:
        a, b = (lst.window(start, count, origin) for lst in lists)
        assert np.array_equal(a, b), (start, count)


# ---------------------------------------------------------------------------
# onc_payload_slots + onc_place_payloads
# ---------------------------------------------------------------------------
def _slots(R, codec, c, what):
    """onc_payload_slots of Call descriptors whose payloads are the case's
    slices, packed at align 1 == the model; -> the model's outputs."""
    n = len(c["pay_len"])
    msgs, status = TP._synth_msgs(c["pay_pos"], c["pay_len"], HM.HEAD_FULL, n)
    want = TP._check_slots(R, codec, msgs, status, 1, HM.HEAD_FULL, None, None, what)
    assert np.array_equal(want["slot_off"], PM.pack_slots(c["pay_len"], 1))
    assert np.array_equal(want["pay_len"], c["pay_len"])
    assert np.array_equal(want["pay_pos"][c["pay_len"] > 0], c["pay_pos"][c["pay_len"] > 0])
    return want


def _place(R, codec, c, want, cap, origin):
    h = None if c["rec_frag"] is None else c
    return TP._place(R, codec, c["wire"], c["frag_start"], c["frag_len"], h, want["pay_pos"], want["pay_len"],
                     want["slot_off"], cap, origin, rec_len=c["rec_len"])


@pytest.mark.parametrize("kind,ntiles,origin,fragmented", TM.PLACE_CASES)
def test_place(R, pair, kind, ntiles, origin, fragmented):
    """Both codecs against the model over dst and its guards: they agree."""
    c = PM.tile_run_records(kind, ntiles, origin, fragmented)
    for codec in pair:
        want = _slots(R, codec, c, f"{kind} {ntiles}")
        done = _place(R, codec, c, want, int(want["slot_off"][-1]), origin)
        assert done == np.nonzero(c["pay_len"])[0].tolist()


@pytest.mark.parametrize("fragmented", [False, True])
@pytest.mark.parametrize("origin", TW.ORIGINS)
@pytest.mark.parametrize("ntiles", CUTS)
def test_place_capacity_cut(R, pair, ntiles, origin, fragmented):
    c, cap = TM.place_cut(ntiles, origin, fragmented)
    slots = PM.pack_slots(c["pay_len"], 1)
    want = {"pay_pos": c["pay_pos"], "pay_len": c["pay_len"], "slot_off": slots}
    for codec in pair:
        done = _place(R, codec, c, want, cap, origin)
        ends = slots[:-1].astype(np.int64) + c["pay_len"]
        assert done == [r for r in np.nonzero(c["pay_len"])[0].tolist() if ends[r] <= cap] and len(done) < len(ends)


# ---------------------------------------------------------------------------
# onc_fragment_iov
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ntiles", TM.FIV_CASES)
def test_fragment_iov(R, pair, kind, ntiles):
    iov, hdr, pay, wire, off = V.tile_run_stream(kind, ntiles)
    recs = [wire[int(a):int(b)] for a, b, hl in zip(off[:-1], off[1:], iov["hdr_len"]) if hl >= 4]
    packed = E.stream_bytes(E.fragment(b"".join(recs), E.offsets_of(recs), V.TILE_RUN_F))
    for codec in pair:
        m = TV._fiv(R, codec, iov, V.TILE_RUN_F)
        assert V.gather(m["pieces"], m["marks"], hdr, pay) == packed


@pytest.mark.parametrize("ntiles", CUTS)
def test_fragment_iov_capacity_cut(R, pair, ntiles):
    iov, cap, W = TM.fragment_iov_cut(ntiles)
    full = V.fragment_iov(iov, V.TILE_RUN_F)
    nf = np.concatenate(([0], np.cumsum([len(V.fragment_iov(iov[i:i + 1], V.TILE_RUN_F)["marks"]) for i in range(len(iov))])))
    r = int(np.searchsorted(full["piece_off"], W, side="right")) - 1       # the first record that does not fit
    for codec in pair:
        m = TV._fiv(R, codec, iov, V.TILE_RUN_F, max_pieces=cap)
        assert len(m["pieces"]) == W
        # the same cut made by the marks' capacity
        m = TV._fiv(R, codec, iov, V.TILE_RUN_F, marks_cap=int(nf[r]) + 2)
        assert len(m["pieces"]) == W


# ---------------------------------------------------------------------------
# onc_defragment_heads: heads_gather's stride loop
# ---------------------------------------------------------------------------
def _heads(R, codec, wire, start, flen, head_len, max_records):
    """test_gpu_heads._check_heads with serial_heads as the model (the stream
    has a record that is too long by its fragments' stated lengths)."""
    nfrag = len(start)
    m = HM.serial_heads(wire, start, flen, head_len, nfrag if max_records is None else max_records)
    g = R.defragment_host_heads(codec, wire, start, flen, head_len, max_records=max_records, fill=SENT)
    n = int(m["result"][0])
    assert g["result"].tolist() == m["result"].tolist()
    raw = g["raw"]
    assert np.array_equal(raw["rec_len"][:n], m["rec_len"]) and (raw["rec_len"][n:] == U32).all()
    assert np.array_equal(raw["status"][:n], m["status"]) and (raw["status"][n:] == -1).all()
    assert np.array_equal(raw["rec_frag"][:n + 1], m["rec_frag"]) and (raw["rec_frag"][n + 1:] == U64).all()
    assert np.array_equal(raw["frag_pre"][:nfrag], m["frag_pre"]) and (raw["frag_pre"][nfrag:] == U64).all()
    want = HM.expected_heads(m, head_len, len(raw["heads"]), SENT)
    bad = np.nonzero(raw["heads"] != want)[0]
    assert len(bad) == 0, (f"heads differ first at byte {bad[0] % head_len} of slot {bad[0] // head_len}: "
                           f"{raw['heads'][bad[:8]]} vs {want[bad[:8]]}")
    return raw["heads"].tobytes()


@pytest.mark.parametrize("max_records", [None, 20, 13, 12])
def test_heads_gather_stride_steps(R, pair, max_records):
    """920 chunks in one workgroup of 256 lanes: four steps, seams in each of
    them, the record that is too long in the third (its slot keeps the
    sentinel), the capacity cut before, at and after it."""
    wire, start, flen, too_long = HM.stride_steps_stream()
    assert too_long == 12
    _both(pair, lambda c: _heads(R, c, wire, start, flen, HM.HEAD_FULL, max_records))
