"""Host model of the tile walk the copy kernels share — defrag_copy
(defrag.hip), frag_copy (fragment.hip), gather_copy (gather.hip), place_copy
(payload.hip) and fragiov_fill (fragment_iov.hip) — and the entry layouts that
put each of its outcomes on a tile that is not the first of its wave's run
(tests/test_tile_walk_model.py on the CPU, tests/test_gpu_tile_runs.py on the
GPU).

Not a test file and not product code: plain Python restating the loop written
down above walk_tiles (onc-rpc_amd/csrc/tile_walk.h), which all five kernels
call. A wave takes a run of `per` consecutive output
tiles. Only the run's first tile searches the sorted positions; every later
tile starts from `ja`, the last entry the tile before handed over, and from a
window of STAGE + 1 consecutive positions from `ja` on:

  research  the tile starts beyond the window (c_lo == STAGE + 1): search on
            from the window's end;
  slide     the window ends inside the tile and does not start at the tile's
            first entry (c_hi == STAGE + 1, k != 0): restart it there;
  global    more than STAGE entries reach into the tile (c_hi == STAGE + 1,
            k == 0): the copy works from global memory, ja = jb;
  staged    the rest: the copy works from the window, ja += c_hi - 1.

Positions here count from the caller's first output byte (entry 0 at or below
0, the last entry — the array's end — at or beyond the written extent W); the
kernels' coordinates count from the 16-byte aligned address `origin` bytes
below it, which is where the tiles are cut. fragiov_fill counts pieces
instead of bytes, at origin 0.
"""
from __future__ import annotations

import bisect
from collections import namedtuple

import numpy as np

STAGE = 128          # k*Stage of the five kernels
WAVES = 4            # waves per workgroup (k*Threads / 64)
MAX_BLOCKS = 2048    # k*MaxBlocks of the five kernels
ONE_GROUP = WAVES    # nw under ONC_VARIANT_COPY_ONE_GROUP

Tile = namedtuple("Tile", "T first retries copy j0 j1 k c_hi")
Tile.__doc__ = """One tile of the walk: its index, whether it is the first of
its wave's run, the retries it made before its copy ('research' / 'slide', in
order), how it was copied ('staged' / 'global'), the entries [j0, j1] handed
to the copy, and the window counts of its last round."""


def took(tile, outcome):
    return outcome == tile.copy or outcome in tile.retries


def default_nw(origin, capacity, tile):
    """Waves of the default launch: a workgroup per WAVES tiles of capacity
    (origin included), at most MAX_BLOCKS."""
    per_wg = tile * WAVES
    return WAVES * min((origin + capacity + per_wg - 1) // per_wg, MAX_BLOCKS)


def runs(ntiles, nw):
    """[(T0, T1)] of the waves that have tiles."""
    per = (ntiles + nw - 1) // nw
    return [(w * per, min(w * per + per, ntiles)) for w in range(nw) if w * per < ntiles]


def _last_at_or_before(e, base, n, x):
    """last_at_or_before(e + base, n, x) of the kernels, literally."""
    lo, hi = 0, n
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if e[base + mid] <= x:
            lo = mid
        else:
            hi = mid
    return lo


def walk(pos, origin, W, tile, nw, stage=STAGE):
    """The walk of every wave over positions `pos` (sorted, duplicates
    allowed) -> [Tile] in tile order."""
    E = [origin + int(p) for p in pos]
    N = len(E) - 1                       # the kernels' nfrag / n / npieces: E[N] closes the array
    assert W > 0 and E[0] <= origin and E[N] >= origin + W and all(a <= b for a, b in zip(E, E[1:]))
    D0, D1 = origin, origin + W
    ntiles = (D1 + tile - 1) // tile
    out = []
    for T0, T1 in runs(ntiles, nw):
        ja = _last_at_or_before(E, 0, N + 1, max(T0 * tile, D0))
        for T in range(T0, T1):
            t0 = T * tile
            lo, hi = max(t0, D0), min(t0 + tile, D1)
            retries = []
            while True:
                win = [E[min(ja + i, N)] for i in range(stage + 1)]
                c_lo = sum(e <= lo for e in win)
                c_hi = sum(e < hi for e in win)
                if c_lo == stage + 1:
                    ja += stage
                    ja += _last_at_or_before(E, ja, N + 1 - ja, lo)
                    retries.append("research")
                    continue
                k = c_lo - 1
                if c_hi == stage + 1 and k != 0:
                    ja += k
                    retries.append("slide")
                    continue
                break
            assert len(retries) <= 3, "the loop above ends after a research, a slide or both"
            if c_hi == stage + 1:
                jb = ja + stage + _last_at_or_before(E, ja + stage, N + 1 - ja - stage, hi - 1)
                out.append(Tile(T, T == T0, tuple(retries), "global", ja, jb, k, c_hi))
                ja = jb
                continue
            out.append(Tile(T, T == T0, tuple(retries), "staged", ja + k, ja + c_hi - 1, k, c_hi))
            ja += c_hi - 1
    return out


def brute(pos, origin, W, tile):
    """Per tile (j0, j1): the last entry at or before the tile's first byte,
    and the last entry before its end."""
    E = [origin + int(p) for p in pos]
    D0, D1 = origin, origin + W
    out = []
    for T in range((D1 + tile - 1) // tile):
        lo, hi = max(T * tile, D0), min(T * tile + tile, D1)
        out.append((bisect.bisect_right(E, lo) - 1, bisect.bisect_left(E, hi) - 1))
    return out


def carried(tiles, outcome):
    """The tiles that took `outcome` and are not the first of their run."""
    return [t.T for t in tiles if not t.first and took(t, outcome)]


# ---------------------------------------------------------------------------
# entry layouts: lists of (length, kind) whose running sum is the positions.
# kind: 'fill' (an ordinary entry), 'zero' (no output), 'short', 'long'.
# ---------------------------------------------------------------------------
class Units:
    """What an entry of one kernel can be: the tile, the range ordinary entries
    are drawn from, the size of a short one, and which lengths exist at all
    (valid(0) holds for all five: an entry of no output)."""

    def __init__(self, tile, fill, short, valid=None):
        self.tile, self.fill, self.short = tile, fill, short
        self.valid = valid or (lambda ln: True)

    def at_least(self, ln):
        while not self.valid(ln):
            ln += 1
        return ln


BYTES = Units(8192, (200, 600), 1)        # defrag_copy, gather_copy, place_copy: any length

KINDS = ("research", "slide", "slide1", "spill", "global", "span")
SIZES = (5, 9, 13)                        # output tiles: per = 2, 3 and 4 with one workgroup
ORIGINS = (0, 1, 15)
# the tile the pile-up stands at: the 2nd (5, 9 tiles) or 3rd (13) of a run of
# the one-workgroup launch; 'global' one earlier at 13 tiles, so that the tile
# after it is carried too
PILE_TILE = {5: 3, 9: 4, 13: 6}
GLOBAL_TILE = {5: 3, 9: 4, 13: 5}
SPAN_START = {5: 0, 9: 3, 13: 4}          # the tile the long entry starts in: the two after it lie inside it
EQUAL_RUN = {5: 129, 9: 300, 13: 257}     # entries of no output at the tile's first byte ('research')
OUTCOME = {"research": "research", "slide": "slide", "slide1": "slide", "spill": "global", "global": "global",
           "span": "staged"}


def layout(kind, ntiles, origin, units=BYTES, seed=0):
    """-> ([(length, kind)], info) of `ntiles` output tiles with `out` at
    `origin` past an aligned address: ordinary entries, and at a tile that is
    carried at nw = ONE_GROUP

      'research': EQUAL_RUN entries of no output exactly at its first byte;
      'slide'   : an entry ending exactly at its first byte, 100 of no output
                  and 60 short ones: the window slides and then holds the tile;
      'slide1'  : an entry ending exactly there and 127 short ones, then one
                  that reaches past the tile: the window slides by one entry;
      'spill'   : 100 of no output and 200 short ones: slide, then global;
      'global'  : an entry across its first byte and 200 short ones (k == 0),
                  an ordinary tile after it;
      'span'    : one entry from the middle of the tile before through the two
                  after it (c_hi - 1 == 0 there), 40 short ones behind it;
      'plain'   : ordinary entries only (ntiles + 1 tiles, for a capacity cut).

    info: 'tile' = that tile, 'W' = the sum."""
    rng = np.random.default_rng(1000 * ntiles + 16 * (KINDS + ("plain",)).index(kind) + origin + seed)
    tile, (flo, fhi) = units.tile, units.fill
    out, pos = [], 0

    def add(ln, what):
        nonlocal pos
        assert units.valid(ln), (ln, what)
        out.append((ln, what))
        pos += ln

    def fill_to(target):
        assert target >= pos
        while pos < target:
            rem = target - pos
            add(int(rng.integers(flo, fhi + 1)) if rem > 2 * fhi else rem // 2 if rem > fhi else rem, "fill")

    def edge(t):
        return t * tile - origin

    total = (ntiles if kind != "plain" else ntiles + 1) * tile - origin - tile // 3
    c = {"global": GLOBAL_TILE, "span": SPAN_START}.get(kind, PILE_TILE).get(ntiles)
    if kind == "research":
        fill_to(edge(c))
        for _ in range(EQUAL_RUN[ntiles]):
            add(0, "zero")
    elif kind in ("slide", "spill"):
        fill_to(edge(c))
        for _ in range(100):
            add(0, "zero")
        for _ in range(60 if kind == "slide" else 200):
            add(units.short, "short")
    elif kind == "slide1":
        fill_to(edge(c))
        for _ in range(STAGE - 1):
            add(units.short, "short")
        add(units.at_least(edge(c + 1) - pos + tile // 4), "long")
    elif kind == "global":
        d = fhi // 4
        fill_to(edge(c) - d)
        add(units.at_least(2 * d), "fill")
        for _ in range(200):
            add(units.short, "short")
    elif kind == "span":
        fill_to(edge(c) + tile // 2)
        add(units.at_least(3 * tile), "long")
        for _ in range(40):
            add(units.short, "short")
        c += 1
    else:
        assert kind == "plain"
    fill_to(max(total, pos + fhi + 1))
    return out, {"tile": c, "W": pos}


def positions(entries):
    """The running sum: len(entries) + 1 positions."""
    return np.concatenate(([0], np.cumsum([ln for ln, _ in entries]))).astype(np.int64)
