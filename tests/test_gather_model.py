"""CPU tests of the host model of onc_piece_offsets / onc_gather_pieces
(tests/gather_model.py): the two loops against fragment_iov_model's own
gather, and a proof that each built piece list has the property its GPU test
(tests/test_gpu_gather.py) names."""
import numpy as np
import pytest

import fragment_iov_model as V
import gather_model as G


def test_model_gathers_fragment_iov_pieces_like_the_writev_model():
    for seed, F in ((3, 1), (4, 7), (5, 16), (6, 1000)):
        iov, hdr, pay, wire, off = V.build(V.random_splits(120, seed), seed=seed)
        m = V.fragment_iov(iov, F)
        src = [np.frombuffer(m["marks"], np.uint8), np.frombuffer(hdr, np.uint8), np.frombuffer(pay, np.uint8)]
        want = V.gather(m["pieces"], m["marks"], hdr, pay)
        pos, res = G.piece_offsets(m["pieces"], G.source_lens(src))
        assert res.tolist() == [len(want), 0, len(m["pieces"])] and int(pos[-1]) == len(want)
        assert G.stream(m["pieces"], src).tobytes() == want
        # any window is the slice of the whole; what lies past the end stays
        for start, count in ((0, 0), (1, 1), (17, 4097), (len(want) - 5, 105), (len(want), 16)):
            out = np.full(count, 0xA5, np.uint8)
            G.gather(m["pieces"], pos, src, start, count, out)
            k = max(0, min(count, len(want) - start))
            assert out[:k].tobytes() == want[start:start + k] and (out[k:] == 0xA5).all()


def test_ok_and_the_saturating_window():
    lens = [10, 0, 1]
    assert G.ok(G.U64, 0, 9, lens) and G.ok(10, 0, 0, lens) and G.ok(0, 10, 0, lens) and G.ok(0, 1, 2, lens)
    assert not G.ok(0, 1, 3, lens) and not G.ok(10, 1, 0, lens) and not G.ok(2, 1, 2, lens)
    assert not G.ok(G.U64, 2, 0, lens) and not G.ok(0, 1, 1, lens) and not G.ok(3, 8, 0, lens)
    src = [np.arange(10, dtype=np.uint8), None, np.array([77], np.uint8)]
    pieces = G.make_pieces([(2, 5, 0), (0, 1, 2), (G.U64, 2, 0), (0, 3, 0)])
    pos, res = G.piece_offsets(pieces, lens)
    assert pos.tolist() == [0, 5, 6, 8, 11] and res.tolist() == [11, 1, 2]
    out = np.full(20, 0xEE, np.uint8)
    G.gather(pieces, pos, src, 3, G.U64, out[:16])              # from + count saturates
    assert out.tolist() == [5, 6, 77, 0xEE, 0xEE, 0, 1, 2] + [0xEE] * 12
    pos0, res0 = G.piece_offsets(G.make_pieces([]), lens)
    assert pos0.tolist() == [0] and res0.tolist() == [0, 0, 0]


def test_one_byte_pieces_fill_tiles_beyond_the_staged_window():
    pieces, src = G.one_byte_pieces()
    assert len(pieces) == 20_000 and (pieces["len"] == 1).all() and set(pieces["src"].tolist()) == {0, 1, 2}
    assert G.pieces_reaching_into_tiles(pieces).min() > G.STAGE
    assert G.piece_offsets(pieces, G.source_lens(src))[1].tolist() == [20_000, 0, 20_000]


@pytest.mark.parametrize("run", [1, 127, 128, 129, 300])
def test_zero_runs_sit_inside_a_tile_and_on_a_boundary(run):
    pieces, src = G.zero_run_list(run)
    runs = G.zero_runs(pieces)
    assert (3000, run) in runs and (2 * G.TILE, run) in runs
    assert 0 < 3000 % G.TILE and (2 * G.TILE) % G.TILE == 0
    assert src[0] is None and G.source_lens(src)[0] == 0           # a NULL base with len 0
    assert G.piece_offsets(pieces, G.source_lens(src))[1][1] == 0  # empty pieces are OK wherever they point
    if run > G.STAGE:
        assert G.pieces_reaching_into_tiles(pieces)[[0, 2]].min() > G.STAGE


def test_long_piece_spans_tiles_and_its_successor_starts_on_a_tiles_last_byte():
    pieces, src = G.long_piece_list()
    pos, res = G.piece_offsets(pieces, G.source_lens(src))
    big = int(np.argmax(pieces["len"]))
    assert int(pieces["len"][big]) == 100_000
    first, last = int(pos[big]) // G.TILE, (int(pos[big + 1]) - 1) // G.TILE
    assert last - first + 1 >= 12
    assert any(int(p) % G.TILE == G.TILE - 1 and int(l) > 1 for p, l in zip(pos[:-1], pieces["len"]))
    assert res[1] == 0 and set(pieces["src"].tolist()) == {0, 1, 2}


def test_alignment_grid_is_complete():
    pieces, src = G.alignment_grid()
    assert G.alignment_pairs(pieces) == {(a, b) for a in range(16) for b in range(16)}
    assert G.piece_offsets(pieces, G.source_lens(src))[1][1] == 0


def test_repeated_and_descending_lists():
    pieces, src = G.repeated_list()
    assert len(pieces) == 5000 and len(set(pieces.tolist())) == 1 and int(pieces["len"][0]) == 7
    assert src[0] is None and src[1] is None
    s = G.stream(pieces, src)
    assert len(s) == 35_000 and s.tobytes() == src[2][13:20].tobytes() * 5000
    pieces, src = G.descending_list()
    for k in (1, 2):
        off = pieces["off"][pieces["src"] == k].astype(np.int64)
        assert len(off) > 100 and (np.diff(off) <= 0).all() and off[0] > off[-1]
    assert G.piece_offsets(pieces, G.source_lens(src))[1][1] == 0


@pytest.mark.parametrize("where", ["first", "last", "mid"])
def test_bad_piece_lists(where):
    pieces, src = G.bad_piece_list(where)
    lens = G.source_lens(src)
    assert tuple(lens) == G.BAD_SRC_LENS
    okv = [G.ok(o, l, s, lens) for o, l, s in pieces.tolist()]
    bad = [i for i, v in enumerate(okv) if not v]
    assert len(bad) == 5
    pos, res = G.piece_offsets(pieces, lens)
    assert res.tolist() == [int(pieces["len"].astype(np.int64).sum()), 5, bad[0]]
    if where == "first":
        assert bad[0] == 0
    elif where == "last":
        assert bad[-1] == len(pieces) - 1
    else:
        assert 0 < int(pos[bad[0]]) < G.TILE and int(pos[bad[2]]) < G.TILE < int(pos[bad[4] + 1])
    # a bad piece points past its source's end only: nothing of it could be read
    for i in bad:
        o, l, s = pieces[i].tolist()
        assert s > 2 or o + l > lens[s]
    # the zero-length piece at an impossible offset is OK
    z = [i for i, (o, l, s) in enumerate(pieces.tolist()) if l == 0]
    assert len(z) == 1 and okv[z[0]] and int(pieces["off"][z[0]]) == G.U64
    # their bytes stay, the neighbours' are written
    out = G.stream(pieces, src, fill=0xA5)
    for i in bad:
        assert (out[int(pos[i]):int(pos[i + 1])] == 0xA5).all()
