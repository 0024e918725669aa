"""The walk model (tests/tile_walk_model.py, of walk_tiles in
onc-rpc_amd/csrc/tile_walk.h) pinned by property, and the proof
that every case tests/test_gpu_tile_runs.py runs reaches the outcome it is
named for on a tile that is not the first of its wave's run — in one
workgroup, and on no tile of the default grid. No GPU."""
import numpy as np
import pytest

import fragment_encode_model as E
import fragment_iov_model as V
import fragment_model as M
import gather_model as G
import heads_model as HM
import payload_model as PM
import tile_walk_model as TW


# ---------------------------------------------------------------------------
# 1. the walk hands every tile the brute-force range
# ---------------------------------------------------------------------------
def _random_positions(seed, tile, ntiles):
    """Sorted positions over about `ntiles` tiles: runs of equal positions of
    1, 127, 128, 129 and 300 entries (some exactly at a tile's first byte),
    single entries spanning several tiles, stretches of more than 128 entries
    in a tile, and ordinary entries."""
    rng = np.random.default_rng(seed)
    pos, lens = 0, []
    runs = [1, 127, 128, 129, 300]
    rng.shuffle(runs)
    while pos < ntiles * tile or runs:
        what = int(rng.integers(0, 8))
        if what == 0 and runs:
            lens.append(1)                               # (the run starts behind an entry that has a byte ...
            pos += 1
            if rng.integers(0, 2):                       # bring the run to a tile's first byte (origin 0)
                lens.append(tile - pos % tile)
            lens += [0] * (runs.pop() - 1) + [2]         # ... and its last entry has bytes)
        elif what == 1:
            lens.append(int(rng.integers(2 * tile, 4 * tile)))
        elif what == 2:
            lens += rng.integers(0, max(2, tile // 300), 200).tolist()
        else:
            lens += rng.integers(1, max(3, tile // 12), int(rng.integers(1, 30))).tolist()
        pos = sum(lens)
    return np.concatenate(([0], np.cumsum(lens))).tolist()


@pytest.mark.parametrize("tile", [512, 8192])
def test_walk_hands_over_the_brute_force_range(tile):
    seen = set()
    for seed in range(6):
        pos = _random_positions(seed, tile, 14)
        eq = np.diff(np.nonzero(np.diff(pos + [pos[-1] + 1]))[0], prepend=-1)      # lengths of the runs of equal positions
        assert {127, 128, 129, 300} <= set(eq.tolist()) and max(np.diff(pos)) >= 2 * tile
        for origin in range(16):
            for W in (pos[-1], pos[-1] - tile // 2 - 3):
                want = TW.brute(pos, origin, W, tile)
                assert max(j1 - j0 for j0, j1 in want) > TW.STAGE
                for nw in (1, 4, 8192):
                    tiles = TW.walk(pos, origin, W, tile, nw)
                    assert [t.T for t in tiles] == list(range(len(want)))
                    for t, (j0, j1) in zip(tiles, want):
                        assert (t.j0, t.j1) == (j0, j1), (seed, origin, nw, t)
                        if t.first:                      # found by the search: no retry, the window starts at the entry
                            assert t.retries == () and t.k == 0
                        seen |= {(o, t.first) for o in t.retries + (t.copy,)}
                    if nw == 8192:
                        assert all(t.first for t in tiles)
    assert seen == {("research", False), ("slide", False), ("global", False), ("staged", False), ("global", True),
                    ("staged", True)}


def test_runs_of_one_workgroup():
    """5-8 tiles: runs of 2; 9: of 3, one wave idle; 13: of 4, the last run short."""
    assert TW.runs(5, 4) == [(0, 2), (2, 4), (4, 5)] and TW.runs(8, 4) == [(0, 2), (2, 4), (4, 6), (6, 8)]
    assert TW.runs(9, 4) == [(0, 3), (3, 6), (6, 9)]
    assert TW.runs(13, 4) == [(0, 4), (4, 8), (8, 12), (12, 13)]
    assert TW.runs(13, TW.default_nw(15, 13 * 8192, 8192)) == [(t, t + 1) for t in range(13)]
    # the default grid runs more than one tile per wave only beyond 8192 tiles
    assert TW.default_nw(0, 1 << 40, 8192) == 8192


# ---------------------------------------------------------------------------
# 2. every built case reaches its outcome on a carried tile in one workgroup,
#    and not at the default grid
# ---------------------------------------------------------------------------
def _check(kind, ntiles, pos, origin, W, cap, tile=8192):
    """The walk of the case in one workgroup and at the default grid (a
    workgroup per four tiles of `cap`)."""
    assert (origin + W + tile - 1) // tile == ntiles, (kind, ntiles, origin, W)
    one = TW.walk(pos, origin, W, tile, TW.ONE_GROUP)
    nw = TW.default_nw(origin, cap, tile)
    dflt = TW.walk(pos, origin, W, tile, nw)
    want = TW.brute(pos, origin, W, tile)
    assert [(t.j0, t.j1) for t in one] == want == [(t.j0, t.j1) for t in dflt]
    assert all(t.first for t in dflt) and not any(t.retries for t in dflt), "the default grid carries nothing"
    if kind in TW.OUTCOME:
        name = TW.OUTCOME[kind]
        c = {"global": TW.GLOBAL_TILE, "span": {n: a + 1 for n, a in TW.SPAN_START.items()}}.get(kind, TW.PILE_TILE)[ntiles]
        assert c in TW.carried(one, name), (kind, ntiles, origin, one[c])
        assert TW.carried(dflt, name) == []
        t = one[c]
        if kind == "research":
            assert t.retries == ("research",) and t.copy == "staged"
        elif kind in ("slide", "slide1"):
            assert t.retries == ("slide",) and t.copy == "staged"
            assert (t.j1 - t.j0 == TW.STAGE - 1) == (kind == "slide1")
        elif kind == "spill":
            assert t.retries == ("slide",) and t.copy == "global"
        elif kind == "global":
            assert t.retries == () and t.k == 0
            if ntiles > 5:                               # the tile after it starts from ja = jb
                assert not one[c + 1].first and one[c + 1].retries == () and one[c + 1].copy == "staged"
        elif kind == "span":                             # c_hi - 1 == 0: ja stays, twice where the run is long enough
            assert t.c_hi == 1 and t.j0 == t.j1 == one[c - 1].j1
            assert one[c + 1].c_hi == 1 and (one[c + 1].first or ntiles > 5)
            assert one[c + 2].j0 == t.j0 and one[c + 2].j1 > t.j1
    return one


CASES = [(k, n, o) for k in TW.KINDS for n in TW.SIZES for o in TW.ORIGINS]
CUTS = (5, 6, 9, 13)       # tiles written when the capacity cuts: the last one carried (6, 9) or a run of its own (5, 13)


def _cut_shape(one, ntiles):
    last = one[-1]
    assert last.T == ntiles - 1 and last.first == (ntiles in (5, 13))


@pytest.mark.parametrize("kind,ntiles,origin", CASES)
def test_layouts(kind, ntiles, origin):
    entries, info = TW.layout(kind, ntiles, origin)
    _check(kind, ntiles, TW.positions(entries), origin, info["W"], info["W"])


@pytest.mark.parametrize("kind,ntiles,origin", CASES)
def test_defragment_cases(kind, ntiles, origin):
    buf, entries = M.tile_run_stream(kind, ntiles, origin)
    pos = M.fragment_out_offsets(buf).tolist() + [int(M.defragment(buf, M.frame_fragments(buf)[0])["rec_off"][-1])]
    assert pos == TW.positions(entries).tolist()
    _check(kind, ntiles, pos, origin, pos[-1], pos[-1])


def defragment_cut(ntiles, origin):
    """(stream, out_cap, W): ordinary records of ntiles + 1 tiles; the capacity
    ends in tile ntiles - 1, and so does the last record that fits."""
    buf, _ = M.tile_run_stream("plain", ntiles, origin)
    cap = ntiles * M.TILE - origin - M.TILE // 3
    ro = M.defragment(buf, M.frame_fragments(buf)[0])["rec_off"].astype(np.int64)
    W = int(ro[ro <= cap].max())
    assert W < cap < int(ro[-1])
    return buf, cap, W


@pytest.mark.parametrize("origin", TW.ORIGINS)
@pytest.mark.parametrize("ntiles", CUTS)
def test_defragment_cut(ntiles, origin):
    buf, cap, W = defragment_cut(ntiles, origin)
    pos = M.fragment_out_offsets(buf).tolist() + [int(M.defragment(buf, M.frame_fragments(buf)[0])["rec_off"][-1])]
    _cut_shape(_check("plain", ntiles, pos, origin, W, cap), ntiles)


@pytest.mark.parametrize("kind,ntiles,origin", CASES)
def test_fragment_cases(kind, ntiles, origin):
    wire, off = E.tile_run_stream(kind, ntiles, origin)
    m = E.fragment(wire, off, E.TILE_RUN_FRAG)
    pos = m["out_off"].astype(np.int64).tolist()
    assert int(m["result"][2]) > 0 or kind not in ("span", "slide1")      # records of several fragments
    _check(kind, ntiles, pos, origin, pos[-1], pos[-1])


def fragment_cut(ntiles, origin):
    wire, off = E.tile_run_stream("plain", ntiles, origin)
    cap = ntiles * E.TILE - origin - E.TILE // 3
    oo = E.fragment(wire, off, E.TILE_RUN_FRAG)["out_off"].astype(np.int64)
    W = int(oo[oo <= cap].max())
    assert W < cap < int(oo[-1])
    return wire, off, cap, W


@pytest.mark.parametrize("origin", TW.ORIGINS)
@pytest.mark.parametrize("ntiles", CUTS)
def test_fragment_cut(ntiles, origin):
    wire, off, cap, W = fragment_cut(ntiles, origin)
    pos = E.fragment(wire, off, E.TILE_RUN_FRAG)["out_off"].astype(np.int64).tolist()
    _cut_shape(_check("plain", ntiles, pos, origin, W, cap), ntiles)


@pytest.mark.parametrize("kind,ntiles,origin", CASES)
def test_gather_cases(kind, ntiles, origin):
    pieces, sources = G.tile_run_list(kind, ntiles, origin)
    pos, res = G.piece_offsets(pieces, G.source_lens(sources))
    assert int(res[1]) == 0
    pos = pos.astype(np.int64).tolist()
    _check(kind, ntiles, pos, origin, pos[-1], pos[-1])


def gather_windows(ntiles, origin):
    """[(from, count)] over G.tile_run_list('research', ntiles, origin), whose
    run of empty pieces stands at stream position P: windows from 0, from one
    and two tiles on (the run again at a tile's first byte, another tile) and
    from the middle of a tile, each to one byte before P, to P, to one byte
    past it, to the stream's end and beyond it; and windows that start at P
    and one byte before it."""
    pieces, _ = G.tile_run_list("research", ntiles, origin)
    pos = np.concatenate(([0], np.cumsum(pieces["len"].astype(np.int64))))
    total = int(pos[-1])
    P = TW.PILE_TILE[ntiles] * G.TILE - origin
    assert (pos == P).sum() == TW.EQUAL_RUN[ntiles] + 1
    out = [(P, 6 * G.TILE), (P - 1, 6 * G.TILE)]
    for start in (0, G.TILE, 2 * G.TILE, G.TILE + 4000):
        out += [(start, end - start) for end in (P - 1, P, P + 1, total, total + 100)]
    return out, P, total


def test_gather_windows():
    """Over the sizes and origins the windows reach, in one workgroup: the
    research on a carried tile of a window that does not start at 0; a window
    that ends in the run, in a carried tile (the capacity cut); a window that
    starts in the run and goes on through carried tiles."""
    reached = set()
    for ntiles in TW.SIZES:
        for origin in TW.ORIGINS:
            pieces, _ = G.tile_run_list("research", ntiles, origin)
            pos = np.concatenate(([0], np.cumsum(pieces["len"].astype(np.int64))))
            windows, P, total = gather_windows(ntiles, origin)
            for start, count in windows:
                W = min(count, total - start)
                rel = (pos - start).tolist()
                one = TW.walk(rel, origin, W, G.TILE, TW.ONE_GROUP)
                dflt = TW.walk(rel, origin, W, G.TILE, TW.default_nw(origin, count, G.TILE))
                want = TW.brute(rel, origin, W, G.TILE)
                assert [(t.j0, t.j1) for t in one] == want == [(t.j0, t.j1) for t in dflt]
                assert all(t.first for t in dflt)
                if start and TW.carried(one, "research"):
                    reached.add("research, from > 0")
                if abs(start + W - P) <= 1 and not one[-1].first:
                    reached.add("ends in the run, carried")
                if start == P and len(one) > 4:
                    reached.add("starts in the run")
    assert reached == {"research, from > 0", "ends in the run, carried", "starts in the run"}


# (the slots do not depend on the form: the fragmented one at one origin)
PLACE_CASES = [c + (False,) for c in CASES] + [(k, n, 0, True) for k in TW.KINDS for n in TW.SIZES]


@pytest.mark.parametrize("kind,ntiles,origin,fragmented", PLACE_CASES)
def test_place_cases(kind, ntiles, origin, fragmented):
    c = PM.tile_run_records(kind, ntiles, origin, fragmented)
    n = len(c["pay_len"])
    slots = PM.pack_slots(c["pay_len"], 1)
    pos = PM.walk_positions(slots, n)
    cap = int(slots[n])
    assert cap == PM.payload_extent(slots, c["pay_len"], cap)
    # entry 0 stands in front of record 0: the walk's entries are one further on than the layout's
    _check(kind, ntiles, pos, origin, cap, cap)
    if fragmented:
        assert (np.diff(c["rec_frag"].astype(np.int64)) > 1).sum() > n // 3
        assert (c["frag_len"] == 4).sum() > 10


def place_cut(ntiles, origin, fragmented):
    c = PM.tile_run_records("plain", ntiles, origin, fragmented)
    return c, ntiles * PM.TILE - origin - PM.TILE // 3


@pytest.mark.parametrize("origin", TW.ORIGINS)
@pytest.mark.parametrize("ntiles", CUTS)
def test_place_cut(ntiles, origin):
    c, cap = place_cut(ntiles, origin, False)
    n = len(c["pay_len"])
    slots = PM.pack_slots(c["pay_len"], 1)
    assert cap < int(slots[n])
    W = PM.payload_extent(slots, c["pay_len"], cap)
    assert W == cap
    _cut_shape(_check("plain", ntiles, PM.walk_positions(slots, n), origin, W, cap), ntiles)


FIV_CASES = [(k, n) for k in TW.KINDS for n in TW.SIZES]


@pytest.mark.parametrize("kind,ntiles", FIV_CASES)
def test_fragment_iov_cases(kind, ntiles):
    iov = V.tile_run_stream(kind, ntiles)[0]
    m = V.fragment_iov(iov, V.TILE_RUN_F)
    pos = m["piece_off"].astype(np.int64).tolist()
    entries, _ = TW.layout(kind, ntiles, 0, V.tile_run_units())
    assert pos == TW.positions(entries).tolist()
    _check(kind, ntiles, pos, 0, pos[-1], pos[-1], tile=V.TILE)
    assert V.ENC_BAD_DESCRIPTOR in m["status"].tolist() or kind not in ("research", "slide", "spill")


def fragment_iov_cut(ntiles):
    iov = V.tile_run_stream("plain", ntiles)[0]
    cap = ntiles * V.TILE - V.TILE // 3
    po = V.fragment_iov(iov, V.TILE_RUN_F)["piece_off"].astype(np.int64)
    W = int(po[po <= cap].max())
    assert W <= cap < int(po[-1])
    return iov, cap, W


@pytest.mark.parametrize("ntiles", CUTS)
def test_fragment_iov_cut(ntiles):
    iov, cap, W = fragment_iov_cut(ntiles)
    pos = V.fragment_iov(iov, V.TILE_RUN_F)["piece_off"].astype(np.int64).tolist()
    _cut_shape(_check("plain", ntiles, pos, 0, W, cap, tile=V.TILE), ntiles)


# ---------------------------------------------------------------------------
# 3. what the older boundary streams reach at the default grid
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [0, 1, 15])
@pytest.mark.parametrize("kind", ["search", "slide", "spill"])
def test_tile_boundary_stream_at_the_default_grid(kind, origin):
    """Three tiles: at the default grid, and in one workgroup as well, every
    tile is the first of its run. No window is restarted; 'spill' copies tile
    1 from global memory."""
    buf = M.tile_boundary_stream(kind, origin)
    pos = M.fragment_out_offsets(buf).tolist() + [int(M.defragment(buf, M.frame_fragments(buf)[0])["rec_off"][-1])]
    for nw in (TW.ONE_GROUP, TW.default_nw(origin, pos[-1], M.TILE)):
        tiles = TW.walk(pos, origin, pos[-1], M.TILE, nw)
        assert len(tiles) == 3 and all(t.first and t.retries == () for t in tiles)
        assert [t.copy for t in tiles] == ["staged", "global" if kind == "spill" else "staged", "staged"]


# ---------------------------------------------------------------------------
# 4. heads_gather's stride loop
# ---------------------------------------------------------------------------
def test_stride_steps_stream():
    wire, start, flen, too_long = HM.stride_steps_stream()
    m = HM.serial_heads(wire, start, flen, HM.HEAD_FULL, 20)
    chunks = 20 * HM.HEAD_FULL // 16
    assert int(m["result"][0]) == 20 and chunks == 920 and -(-chunks // HM.GATHER_GROUP) == 4
    # by default the grid covers min(nfrag, max_records) slots: one step
    assert len(start) >= 20
    assert m["status"].tolist() == [HM.ENC_TOO_LONG if r == too_long else HM.OK for r in range(20)]
    assert m["rec_len"][too_long] == 0 and m["slots"][too_long] is None
    step = lambda r: r * HM.HEAD_FULL // 16 // HM.GATHER_GROUP
    assert step(too_long) == 2
    # records of many fragments in every step from the second on
    nf = np.diff(m["rec_frag"].astype(np.int64))
    assert {step(r) for r in range(20) if nf[r] > 100} >= {1, 2, 3}
    # apart from the record that is too long, the stream is an ordinary one: the other model agrees
    keep = [j for j in range(len(start)) if not int(m["rec_frag"][too_long]) <= j < int(m["rec_frag"][too_long + 1])]
    a = HM.defragment_heads(wire, start[keep], flen[keep], HM.HEAD_FULL)
    b = HM.serial_heads(wire, start[keep], flen[keep], HM.HEAD_FULL, 19)
    assert HM.same_heads(a, b) == []
