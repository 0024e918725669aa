"""The host model of onc_fragment (tests/fragment_encode_model.py) checked
against the existing, independent statement of the same cut
(fragment_model.refragment with fixed_cuts) and against the models of the
receive side (frame_fragments, defragment), and the preconditions of every
stream tests/test_gpu_fragment_encode.py builds: each provably has the
property its GPU test names. CPU only."""
import numpy as np
import pytest

import fragment_encode_model as E
import fragment_model as M
import frame_model as FM


@pytest.fixture(scope="module", autouse=True)
def symbol():
    """The model stands for a call of the library: without it there is
    nothing these tests describe."""
    import onc_rpc_amd.runtime as R
    assert hasattr(R.load_library(), "onc_fragment") and "onc_fragment" in R.EXPORTED


@pytest.mark.parametrize("max_frag", E.GOLDEN_MAX_FRAGS)
def test_model_against_refragment_and_the_receive_side(golden, max_frag):
    wire, off = M.golden_stream(golden)
    assert (len(off) - 1, len(wire)) == (40, 3633)
    m = E.fragment(wire, off, max_frag)
    out = E.stream_bytes(m)
    assert out == M.refragment(wire, off, M.fixed_cuts(max_frag))
    assert not m["status"].any() and int(m["out_off"][-1]) == len(out) == int(m["result"][1])
    fo, n, consumed, st, _, _ = M.frame_fragments(out)
    assert (st, consumed, n) == (M.OK, len(out), int(m["result"][0]))
    d = M.defragment(out, fo)
    assert b"".join(d["records"]) == wire and np.array_equal(d["rec_off"], off)
    assert int(d["result"][5]) == int(m["result"][2])
    want = {1: (3474, 17369, 39), 16: (237, 4421, 36), E.MAX_FRAG_LIMIT: (40, 3633, 0)}.get(max_frag)
    if want:
        assert tuple(m["result"].tolist()) == want
    if max_frag == E.MAX_FRAG_LIMIT:
        assert out == wire and np.array_equal(m["out_off"], off)


def test_model_statuses_and_capacity():
    wire, off = E.non_record_extents("mixed")
    m = E.fragment(wire, off, 16)
    lens = np.diff(off.astype(np.int64))
    assert set(lens[lens < 4].tolist()) == {0, 1, 2, 3}
    assert m["status"].tolist() == [E.OK if l == 0 or l >= 4 else E.ENC_BAD_DESCRIPTOR for l in lens]
    assert all((r is None) == (l < 4) for r, l in zip(m["records"], lens))
    # a record of 20 body bytes at max_frag 16: 16 + 4
    assert m["records"][2][:4] == b"\x00\x00\x00\x10" and m["records"][2][20:24] == b"\x80\x00\x00\x04"
    assert m["records"][6] == b"\x80\x00\x00\x00"
    need = int(m["out_off"][-1])
    first = int(m["out_off"][8])                          # the 40-byte body's record
    for cap, n_ok in ((need, 4), (need - 1, 3), (first + 30, 2), (first, 2), (0, 0)):
        c = E.fragment(wire, off, 16, cap)
        assert np.array_equal(c["out_off"], m["out_off"]) and np.array_equal(c["result"], m["result"])
        st = c["status"][lens >= 4].tolist()
        assert st == [E.OK] * n_ok + [E.ENC_WRITE_ZERO] * (4 - n_ok), (cap, st)
        assert c["status"][lens < 4].tolist() == m["status"][lens < 4].tolist()
    only = E.fragment(*E.non_record_extents("only"), 5)
    assert only["result"].tolist() == [0, 0, 0] and not only["out_off"].any()
    empty = E.fragment(b"", np.zeros(1, np.uint64), 5)
    assert empty["result"].tolist() == [0, 0, 0] and empty["out_off"].tolist() == [0]


def test_alignment_stream_covers_every_source_and_destination_alignment():
    wire, off = E.alignment_stream()
    bodies = np.diff(off.astype(np.int64)) - 4
    assert set(E.ALIGN_BODIES) <= set(bodies.tolist()) and bodies.max() >= 16 * 17
    pairs = set()
    for F in E.ALIGN_MAX_FRAGS:
        pairs |= E.fast_path_pairs(off, F)
    assert pairs == {(s, d) for s in range(16) for d in range(16)}
    # what a shift sees alone: every destination placement meets several sources
    assert all(len(E.fast_path_pairs(off, 100, [sh])) >= 4 for sh in range(16))


@pytest.mark.parametrize("F", E.COUNT_EDGE_FS)
def test_count_edges_stream(F):
    wire, off = E.count_edges_stream(F)
    bodies = sorted(set((np.diff(off.astype(np.int64)) - 4).tolist()))
    assert bodies == sorted({0, F - 1, F, F + 1, 2 * F, 2 * F + 1})
    m = E.fragment(wire, off, F)
    ks = {int(b): len(M.frame_fragments(r)[0]) - 1 for b, r in zip(np.diff(off.astype(np.int64)) - 4, m["records"])}
    assert ks[0] == 1 and ks[F] == 1 and ks[F + 1] == 2 and ks[2 * F] == 2 and ks[2 * F + 1] == 3
    assert E.stream_bytes(m) == M.refragment(wire, off, M.fixed_cuts(F))


def test_many_records_per_tile_streams():
    wire, off = E.empty_records_stream()
    m = E.fragment(wire, off, 8)
    assert E.records_reaching_into_tiles(m).max() > 2000 > E.STAGE
    assert E.stream_bytes(m) == M.refragment(wire, off, M.fixed_cuts(8))
    wire, off = E.short_records_stream()
    m = E.fragment(wire, off, 8)
    assert len(off) - 1 == 500 and (np.diff(off.astype(np.int64)) == 24).all()
    assert m["result"].tolist() == [1500, 500 * 32, 500]
    assert E.records_reaching_into_tiles(m).max() > E.STAGE


@pytest.mark.parametrize("max_frag,frags", [(7, 14286), (8188, 13), (70_001, 2), (100_000, 1)])
def test_large_record_stream(max_frag, frags):
    wire, off = E.large_record_stream()
    m = E.fragment(wire, off, max_frag)
    assert int(m["result"][0]) == frags + 2 * max(1, -(-24 // max_frag))       # and the two 28-byte replies
    assert int(m["out_off"][-1]) > 3 * E.TILE
    assert E.stream_bytes(m) == M.refragment(wire, off, M.fixed_cuts(max_frag))


@pytest.mark.parametrize("origin", [0, 1, 15])
def test_tile_boundary_streams(origin):
    F = E.TILE_MARK_FRAG
    for d in range(5):
        m = E.fragment(*E.tile_mark_stream(d, origin), F)
        pos, cont = E.mark_positions(m, F)
        assert (E.TILE - origin - d) in pos[cont].tolist()
    m = E.fragment(*E.tile_record_boundary_stream(origin), F)
    assert (E.TILE - origin) in m["out_off"].tolist()
    assert int(m["out_off"][-1]) + origin > E.TILE + 2000


def test_non_record_extents_and_block_edges():
    wire, off = E.non_record_extents("mixed")
    lens = np.diff(off.astype(np.int64)).tolist()
    assert lens[0] == 0 and lens[-1] == 0 and 0 < lens[1] < 4          # first, last
    assert any(0 < a < 4 and 0 < b < 4 for a, b in zip(lens, lens[1:]))   # adjacent
    assert all(l < 4 for l in np.diff(E.non_record_extents("only")[1].astype(np.int64)))
    for n in (255, 256, 257, 1025):
        w, o = E.short_records(n)
        assert len(o) - 1 == n and (np.diff(o.astype(np.int64)) >= 4).all()
        assert E.stream_bytes(E.fragment(w, o, 9)) == M.refragment(w, o, M.fixed_cuts(9))
