"""The host model of fragment framing and reassembly
(tests/fragment_model.py) checked against the oracle's encoder and framer,
and the preconditions of every stream tests/test_gpu_fragments.py builds:
each provably has the property its GPU test names. CPU only."""
import numpy as np
import pytest

import fragment_model as M
import frame_model as FM
import onc_rpc_amd.synth as S


def _streams(oracle, golden):
    wire, off = M.golden_stream(golden)
    assert len(off) - 1 >= 40
    yield wire, off
    w, o, st, _ = oracle.encode_batch(S.mixed(300, seed=5, pmin=0, pmax=700))
    assert not st.any()
    yield w, o


def test_refragment_then_reassemble_gives_back_the_stream(oracle, golden):
    for wire, off in _streams(oracle, golden):
        for seed in (1, 2, 3):
            frag = M.refragment(wire, off, M.random_cuts(seed))
            fo, n, consumed, st, _, _ = M.frame_fragments(frag)
            assert (consumed, st) == (len(frag), M.OK) and n >= len(off) - 1
            m = M.defragment(frag, fo)
            assert b"".join(m["records"]) == wire
            assert np.array_equal(m["rec_off"], np.asarray(off, np.uint64))
            assert not m["status"].any()
            per = M.fragments_per_record(frag)
            assert m["result"].tolist() == [len(off) - 1, len(frag), len(wire), 0, 0, int((per > 1).sum())]
            assert (per > 1).any() and (np.diff(fo.astype(np.int64)) == 4).any(), "multi-fragment and empty fragments"
        # every 8 bytes: a record of n body bytes comes in ceil(n / 8) fragments
        frag = M.refragment(wire, off, M.fixed_cuts(8))
        m = M.defragment(frag, M.frame_fragments(frag)[0])
        assert b"".join(m["records"]) == wire


def test_fragment_framing_is_record_framing_when_every_mark_is_last(oracle, golden):
    for wire, off in _streams(oracle, golden):
        for buf, m in ((wire, None), (wire[:-3], None), (wire[:len(wire) // 2], None), (wire, 7), (wire, 0)):
            fo, n, consumed, st, a0, a1 = M.frame_fragments(buf, m)
            o = oracle.frame_stream(buf, m)
            assert (n, consumed, st, a0, a1) == o[1:]
            assert np.array_equal(fo, o[0])
        # clearing last bits moves no offset, and never stops the loop
        fo = M.frame_fragments(wire)[0]
        cleared = M.clear_last_bits(wire, fo, range(1, len(fo) - 1, 3))
        assert np.array_equal(M.frame_fragments(cleared)[0], fo)
        assert oracle.frame_stream(cleared)[3] == M.FRAGMENTED


def test_model_statuses_pending_and_capacity():
    buf, head = M.pending_stream()
    fo, n, consumed, st, _, _ = M.frame_fragments(buf)
    assert (consumed, st) == (len(buf), M.OK)
    m = M.defragment(buf, fo)
    assert m["result"].tolist() == [3, head, int(m["rec_off"][3]), 3, 90, 1]
    end1 = int(m["rec_off"][2])
    for cap, want in ((end1 - 1, [0, 105, 105]), (end1, [0, 0, 105]), (0, [105, 105, 105])):
        c = M.defragment(buf, fo, cap)
        assert c["status"].tolist() == want
        assert np.array_equal(c["rec_off"], m["rec_off"]), "placement ignores the capacity"
        assert [r is None for r in c["records"]] == [s != 0 for s in want]
    assert M.defragment(b"", [0])["result"].tolist() == [0] * 6
    # an empty record: the bare mark
    e = M.shapes_stream("empty")
    m = M.defragment(e, M.frame_fragments(e)[0])
    assert m["records"][0] == b"\x80\x00\x00\x00" and m["records"][2] == b"\x80\x00\x00\x00"


# ---------------------------------------------------------------------------
# the streams of tests/test_gpu_fragments.py
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("span", [0, 1, 5])
def test_continuation_stream_spans(span):
    buf = M.continuation_stream(span)
    assert M.frame_fragments(buf)[2:4] == (len(buf), M.OK)
    assert M.whole_chunks_inside_a_fragment(buf, M.EDGE_CHUNK) == span
    assert FM.true_starts(buf)[2] == FM.FRAGMENTED, "record framing stops at it"


def test_continuation_only_chunks():
    buf = M.continuation_only_stream()
    assert M.frame_fragments(buf)[2:4] == (len(buf), M.OK)
    assert M.chunks_with_only_continuation_starts(buf, M.EDGE_CHUNK) >= 8


def test_more_than_64_starts():
    buf = M.empty_fragments_stream()
    assert M.frame_fragments(buf)[2:4] == (len(buf), M.OK)
    assert M.max_starts_in_a_chunk(buf, 1024) > 64
    # and at 64-byte chunks a run of more than 64 starts that no chunk can
    # guess (empty continuation fragments): one chain keeps more than it can
    assert (M.fragments_per_record(buf) > 64).any()


def test_straddling_marks():
    buf = M.straddle_stream()
    assert M.frame_fragments(buf)[2:4] == (len(buf), M.OK)
    assert M.straddle_offsets(buf, M.EDGE_CHUNK) == {-3, -2, -1, 0, 1}


def test_header_lookalikes():
    buf = M.header_lookalike_stream()
    assert M.frame_fragments(buf)[2:4] == (len(buf), M.OK)
    assert M.off_chain_guess_chunks(buf, M.EDGE_CHUNK) >= 6


def test_big_continuation_stream():
    buf = M.big_continuation_stream()
    assert 1 << 20 <= len(buf) < (1 << 20) + (1 << 20)
    assert M.whole_chunks_inside_a_fragment(buf, 65536) >= 3


def test_alignment_coverage():
    buf = M.alignment_stream()
    assert M.alignment_coverage(buf) == {(s, d) for s in range(16) for d in range(16)}
    assert (M.fragments_per_record(buf) == 2).all()
    bodies = np.diff(M.frame_fragments(buf)[0].astype(np.int64)) - 4
    assert set(bodies.tolist()) == set(M.ALIGN_LENS)


def test_shapes():
    per = {w: M.fragments_per_record(M.shapes_stream(w)) for w in M.SHAPES}
    assert per["tiny"].min() >= 2 and (np.diff(M.frame_fragments(M.shapes_stream("tiny"))[0].astype(np.int64)) <= 7).all()
    assert 65 in per["frags65"] and 200 in per["frags200"]
    assert np.diff(M.frame_fragments(M.shapes_stream("huge"))[0].astype(np.int64)).max() > 8 * 8192
    assert per["multi_first"][0] > 1 and per["multi_first"][-1] == 1
    assert per["multi_last"][0] == 1 and per["multi_last"][-1] > 1
    for w in M.SHAPES:
        buf = M.shapes_stream(w)
        assert M.frame_fragments(buf)[2:4] == (len(buf), M.OK) and buf[M.frame_fragments(buf)[0][-2]] & 0x80


@pytest.mark.parametrize("origin", [1, 0, 15])
def test_tile_boundary_streams(origin):
    at = M.TILE - origin
    for kind, (empties, ones) in {"search": (300, 0), "slide": (100, 60), "spill": (100, 200)}.items():
        buf = M.tile_boundary_stream(kind, origin)
        assert M.frame_fragments(buf)[2:4] == (len(buf), M.OK)
        e = M.fragment_out_offsets(buf)
        assert int((e == at).sum()) == empties + 1, "empty fragments, and the one after them, at the tile's first byte"
        in_tile = int(((e > at) & (e < at + M.TILE)).sum())
        assert in_tile in (ones, ones + 1)
        # the window: STAGE + 1 entries from the fragment holding the byte before the tile
        if kind == "search":
            assert empties > M.STAGE, "the tile's first fragment lies beyond the window"
        else:
            assert empties <= M.STAGE < empties + in_tile, "the window ends inside the tile: it slides"
            assert (in_tile > M.STAGE) == (kind == "spill"), "and then holds the tile, or not"
        m = M.defragment(buf, M.frame_fragments(buf)[0])
        assert not m["status"].any() and int(m["result"][0]) == 4
