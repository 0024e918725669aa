"""A piece list written as one stream on the device: onc_piece_offsets and
onc_gather_pieces (gather.hip). Positions and results are compared with the
host model (tests/gather_model.py), the gathered bytes with the model, with
the packed path on the device (onc_encode + onc_fragment) and with its model
over the oracle's encoder, and the stream goes back through the receive side.
tests/test_gather_model.py proves on the CPU that each built piece list has
the property its test names.

`out` is pre-filled with a sentinel and has 64 guard bytes on each side;
piece_pos and result are pre-filled too and one word longer than needed, so a
byte or an entry written where none belongs shows. No extent handed to the
kernels is out of bounds, except the bad pieces the contract says are never
read."""
import functools
import os
import subprocess

import numpy as np
import pytest

import big_wire as BW
import fragment_encode_model as E
import fragment_iov_model as V
import gather_model as G
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
from test_gpu_far_offsets import FAR, G31, G32, SLAB, slab  # noqa: F401  (slab: the 6.5 GiB device slab fixture)
from test_gpu_fragment_iov import _encode_iov
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
def codec(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = R.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_group(R):
    """A codec that launches the copy as one workgroup
    (ONC_VARIANT_COPY_ONE_GROUP): several tiles per wave
    (tests/test_gpu_tile_runs.py)."""
    c = R.Codec(0, variant=R.VARIANT_COPY_ONE_GROUP)
    yield c
    c.close()


def _dev(a):
    """A numpy array's bytes in a device tensor of exactly that size (None: None)."""
    import torch
    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Listed:
    """A piece list and its sources on the device; onc_piece_offsets of it ==
    the model (piece_pos, result, the fill after both)."""

    def __init__(self, R, codec, pieces, sources, d_sources=None, lens=None, d_pieces=None):
        import torch
        self.R, self.codec = R, codec
        self.pieces, self.sources = pieces, sources
        self.n = len(pieces)
        self.lens = G.source_lens(sources) if lens is None else lens
        self.d_sources = [_dev(s) for s in sources] if d_sources is None else d_sources
        self.src = R.gather_src(*[(t, ln) for t, ln in zip(self.d_sources, self.lens)])
        for t in self.d_sources:
            assert t is None or t.data_ptr() % 16 == 0
        self.d_pieces = R.to_device(pieces, "cuda") if d_pieces is None else d_pieces
        self.pos, self.res = G.piece_offsets(pieces, self.lens)
        self.total = int(self.res[0])
        self.d_pos = torch.full((self.n + 2,), -3, dtype=torch.int64, device="cuda")
        d_res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        codec.piece_offsets(self.d_pieces, self.n, self.src, self.d_pos, d_res)
        codec.sync()
        r = d_res.cpu().numpy()
        assert r[:3].view(np.uint64).tolist() == self.res.tolist(), (r.tolist(), self.res.tolist())
        assert r[3] == -1, "result written past its three words"
        p = self.d_pos.cpu().numpy()
        assert np.array_equal(p[:self.n + 1].view(np.uint64), self.pos), "piece_pos"
        assert p[self.n + 1] == -3, "piece_pos written past npieces + 1"
        self._whole = None

    def whole(self):
        """The model's stream, the sentinel where a bad piece stands (computed once)."""
        if self._whole is None:
            out = np.full(self.total, SENT, np.uint8)
            self._whole = G.gather(self.pieces, self.pos, self.sources, 0, self.total, out, self.lens)
            self._whole.setflags(write=False)
        return self._whole

    def expect(self, start, count):
        """out[0, count) after a gather of [start, start + count) into sentinel bytes."""
        want = np.full(count, SENT, np.uint8)
        k = max(0, min(count, self.total - start))
        want[:k] = self.whole()[start:start + k]
        return want

    def window(self, start, count, shift=0, want=None, out=None):
        """onc_gather_pieces of the window into a sentinel-filled buffer `shift`
        bytes past a 16-byte aligned address == the model, guards included.
        Returns the window's bytes."""
        import torch
        want = self.expect(start, count) if want is None else want
        buf = torch.full((16 + GUARD + shift + count + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        lo = (-buf.data_ptr()) % 16 + GUARD + shift
        self.codec.gather_pieces(self.d_pieces, self.d_pos, self.n, self.src, start, count, buf.data_ptr() + lo)
        self.codec.sync()
        got = buf.cpu().numpy()
        full = np.full(got.size, SENT, np.uint8)
        full[lo:lo + count] = want
        bad = np.nonzero(got != full)[0]
        assert len(bad) == 0, (f"window ({start}, {count}) shift {shift}: first difference at window byte "
                               f"{bad[0] - lo} (stream {start + bad[0] - lo}), {len(bad)} in all: "
                               f"{got[bad[:8]]} vs {full[bad[:8]]}")
        return got[lo:lo + count]


# ---------------------------------------------------------------------------
# 1. parity with the packed path
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mixed(n):
    return S.mixed(n, seed=300 + n % 89, pmin=0, pmax=300, exotic=0.2)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_parity_with_the_packed_path(codec, R, oracle, n):
    hb = _mixed(n)
    o_wire, o_off, o_st, _ = oracle.encode_batch(hb)
    o_off = np.asarray(o_off, np.uint64)
    g_wire, g_off, g_st, _ = R.encode_host_batch(codec, hb)               # onc_encode on the device
    assert g_wire == bytes(o_wire) and np.array_equal(g_st, o_st)
    hdr, iov, st, d_iov, _ = _encode_iov(R, codec, hb)
    assert np.array_equal(st, o_st)
    pay = np.asarray(hb.payload_arena, np.uint8)
    d_hdr, d_pay = _dev(hdr), _dev(pay)
    w = np.frombuffer(g_wire + b"\0" * 16, np.uint8).copy()
    for max_frag in E.GOLDEN_MAX_FRAGS:
        marks, pieces, out_off, piece_off, fst, fres = R.fragment_iov_host(codec, iov, max_frag)
        packed = R.fragment_host(codec, g_wire, g_off, max_frag)[0]       # onc_fragment on the device
        model = E.stream_bytes(E.fragment(o_wire, o_off, max_frag))
        assert packed == model
        lst = Listed(R, codec, pieces, [marks if len(marks) else None, hdr, pay],
                     d_sources=[_dev(marks) if len(marks) else None, d_hdr, d_pay])
        assert lst.total == len(model) == int(fres[1]) and int(lst.res[1]) == 0
        assert lst.whole().tobytes() == model, f"the model's gather, n {n} max_frag {max_frag}"
        for shift in (0, 1, 5, 15):
            got = lst.window(0, lst.total, shift)
            assert got.tobytes() == packed, f"n {n} max_frag {max_frag} shift {shift}"
        # and back through the receive side
        rb, ro, rs, rr, rf = R.reassemble_host_stream(codec, got.tobytes())
        assert rb == g_wire and np.array_equal(ro, g_off) and not rs.any(), f"n {n} max_frag {max_frag}"
        for mode in MODES:
            assert_decoded_equal(R.decode_host_wire(codec, np.frombuffer(rb + b"\0" * 16, np.uint8).copy(), ro, mode),
                                 oracle.decode_batch(w, g_off, mode), f"n {n} max_frag {max_frag} mode {mode}")


# ---------------------------------------------------------------------------
# 2. a limit per record
# ---------------------------------------------------------------------------
def test_per_record_limits(codec, R):
    (iov, hdr, pay, wire, off), lim = V.per_record_stream()
    marks, pieces, out_off, piece_off, st, res = R.fragment_iov_host(codec, iov, 16, rec_max_frag=lim)
    invalid = (lim < 1) | (lim > V.MAX_FRAG_LIMIT)
    has_bytes = (iov["hdr_len"].astype(np.int64) + iov["payload_len"]) > 0
    assert (invalid & has_bytes).sum() >= 3
    # every record on its own, cut at its own limit by the packed path's model
    want = []
    for i in range(len(iov)):
        if invalid[i] or not has_bytes[i]:
            assert piece_off[i] == piece_off[i + 1] and out_off[i] == out_off[i + 1]      # contributes nothing
            assert st[i] == (V.ENC_BAD_DESCRIPTOR if has_bytes[i] else V.OK)
            continue
        rec = wire[int(off[i]):int(off[i + 1])]
        want.append(E.stream_bytes(E.fragment(rec, [0, len(rec)], int(lim[i]))))
    want = b"".join(want)
    lst = Listed(R, codec, pieces, [marks, np.frombuffer(hdr, np.uint8), np.frombuffer(pay, np.uint8)])
    assert lst.total == len(want) == int(res[1])
    for shift in (0, 7):
        assert lst.window(0, lst.total, shift).tobytes() == want


# ---------------------------------------------------------------------------
# 3. windows
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def windows_list(codec, R):
    iov, hdr, pay, wire, off = V.build(V.random_splits(300, 81, hmax=60, pmax=420), seed=82)
    m = V.fragment_iov(iov, 100)
    lst = Listed(R, codec, m["pieces"], [np.frombuffer(m["marks"], np.uint8), np.frombuffer(hdr, np.uint8),
                                         np.frombuffer(pay, np.uint8)])
    assert 6 * G.TILE < lst.total < 80_000
    assert lst.whole().tobytes() == E.stream_bytes(E.fragment(wire, off, 100))
    return lst


def test_windows(windows_list):
    lst = windows_list
    total = lst.total
    for start, count in ((0, total), (0, 0), (total, 16), (1, 1), (8191, 2), (8192, 8192), (8185, 8207)):
        for shift in (0, 3):
            lst.window(start, count, shift)
    # starting inside a mark piece
    marks = np.nonzero((lst.pieces["src"] == V.PIECE_MARK) & (lst.pos[:-1] > 9000))[0]
    p = int(lst.pos[marks[0]])
    for d in (1, 2, 3):
        lst.window(p + d, 100, shift=d)
    # running 100 bytes past the end: the tail stays as it was
    got = lst.window(total - 50, 150)
    assert (got[50:] == SENT).all() and got[:50].tobytes() == lst.whole()[total - 50:].tobytes()
    lst.window(total - 1, 101, shift=9)
    lst.window(total + 1, 64)


def test_every_short_window_at_every_alignment(windows_list):
    for count in range(1, 34):
        for shift in range(16):
            windows_list.window(8190, count, shift)


def test_concatenated_windows_are_the_stream(windows_list):
    lst = windows_list
    parts = [lst.window(a, 4097, shift=(a // 4097) % 16) for a in range(0, lst.total, 4097)]
    assert np.concatenate(parts)[:lst.total].tobytes() == lst.whole().tobytes()


# ---------------------------------------------------------------------------
# 4. generic lists
# ---------------------------------------------------------------------------
def _generic(R, codec, pieces, sources, shifts=(0, 5)):
    lst = Listed(R, codec, pieces, sources)
    assert int(lst.res[1]) == 0
    for shift in shifts:
        lst.window(0, lst.total, shift)
    lst.window(4097, lst.total, 11)
    lst.window(G.TILE - 1, G.TILE + 2, 1)
    return lst


def test_one_byte_pieces(codec, R):
    lst = _generic(R, codec, *G.one_byte_pieces())
    assert G.pieces_reaching_into_tiles(lst.pieces).min() > G.STAGE


@pytest.mark.parametrize("run", [1, 127, 128, 129, 300])
def test_zero_length_runs(codec, R, run):
    pieces, sources = G.zero_run_list(run)
    assert sources[0] is None                        # an unused source: NULL base, len 0
    lst = _generic(R, codec, pieces, sources, shifts=(0, 5, 15))
    assert lst.src.base[0] is None and lst.src.len[0] == 0
    # windows that start and end in the runs
    for start in (2999, 3000, 3001, 2 * G.TILE - 1, 2 * G.TILE, 2 * G.TILE + 1):
        lst.window(start, 40, shift=start % 16)
        lst.window(start, G.TILE, shift=0)
    lst.window(0, 3000)
    lst.window(0, 2 * G.TILE)


def test_one_piece_of_many_tiles(codec, R):
    _generic(R, codec, *G.long_piece_list())


def test_many_tiles_in_one_workgroup(codec, one_group, R, windows_list):
    """The lists of this file that are longer than four tiles — one piece of
    13 tiles and the 6-tile list of the window tests — with the copy launched
    as one workgroup: the same bytes as the default launch."""
    pieces, sources = G.long_piece_list()
    lst = _generic(R, one_group, pieces, sources, shifts=(0, 5, 15))
    assert lst.total > 12 * G.TILE
    ref = Listed(R, codec, pieces, sources)
    assert np.array_equal(lst.window(0, lst.total, 1), ref.window(0, lst.total, 1))
    ref = windows_list
    lst = Listed(R, one_group, ref.pieces, ref.sources)
    for start, count in ((0, ref.total), (1, ref.total), (8185, 5 * G.TILE + 15), (G.TILE, ref.total),
                         (ref.total - 5 * G.TILE - 50, 5 * G.TILE + 150)):
        for shift in (0, 3):
            assert np.array_equal(lst.window(start, count, shift), ref.window(start, count, shift))


def test_alignment_grid(codec, R):
    pieces, sources = G.alignment_grid()
    _generic(R, codec, pieces, sources, shifts=(0, 1, 5, 15))


def test_repeated_source_bytes(codec, R):
    _generic(R, codec, *G.repeated_list())


def test_descending_source_order(codec, R):
    lst = _generic(R, codec, *G.descending_list())
    assert set(lst.pieces["src"].tolist()) == {0, 1, 2}


# ---------------------------------------------------------------------------
# 5. bad pieces
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["first", "last", "mid"])
def test_bad_pieces_are_never_read_and_leave_their_bytes(codec, R, where):
    pieces, sources = G.bad_piece_list(where)
    lst = Listed(R, codec, pieces, sources)          # exactly-sized source tensors
    assert lst.res.tolist()[1] == 5 and lst.total == int(pieces["len"].astype(np.int64).sum())
    okv = np.array([G.ok(o, l, s, lst.lens) for o, l, s in pieces.tolist()])
    assert int(lst.res[2]) == int(np.nonzero(~okv)[0][0])
    whole = lst.whole()
    for i in np.nonzero(~okv)[0]:
        assert (whole[int(lst.pos[i]):int(lst.pos[i + 1])] == SENT).all()
    for shift in (0, 1, 8, 15):
        lst.window(0, lst.total, shift)
    # windows that begin and end inside the bad pieces
    for i in np.nonzero(~okv)[0]:
        a = int(lst.pos[i])
        lst.window(a, 64, shift=a % 16)
        lst.window(max(0, a - 37), 40 + int(pieces["len"][i]), shift=3)
        lst.window(a + 1, 1)


# ---------------------------------------------------------------------------
# 6. mapped host output
# ---------------------------------------------------------------------------
def test_mapped_host_output(codec, R, windows_list):
    import torch
    lst = windows_list
    want = lst.window(0, lst.total).tobytes()        # the device run
    size = 3 + lst.total + GUARD
    pinned = torch.full((size,), SENT, dtype=torch.uint8).pin_memory()
    mapped = R.HostMapped(codec, size)
    mapped.host[:] = SENT
    try:
        for name, dev, host in (("pin_memory", R.host_device_pointer(codec, pinned), pinned.numpy()),
                                ("onc_host_register", mapped.data_ptr(), mapped.host)):
            codec.gather_pieces(lst.d_pieces, lst.d_pos, lst.n, lst.src, 0, lst.total, dev + 3)
            codec.sync()
            assert (host[:3] == SENT).all() and (host[3 + lst.total:] == SENT).all(), name
            assert host[3:3 + lst.total].tobytes() == want, name
            host[:] = SENT
            codec.gather_pieces(lst.d_pieces, lst.d_pos, lst.n, lst.src, 8190, 4099, dev + 3)
            codec.sync()
            assert (host[:3] == SENT).all() and (host[3 + 4099:] == SENT).all(), name
            assert host[3:3 + 4099].tobytes() == want[8190:8190 + 4099], name
    finally:
        mapped.close()


# ---------------------------------------------------------------------------
# 7. beyond 4 GiB
# ---------------------------------------------------------------------------
class Sparse:
    """A source of `size` bytes of which only the placed blocks are known."""

    def __init__(self, size, blocks):
        self.size, self.blocks = size, blocks

    def __len__(self):
        return self.size

    def __getitem__(self, s):
        for base, data in self.blocks:
            if base <= s.start and s.stop <= base + len(data):
                return data[s.start - base:s.stop - base]
        raise AssertionError(f"bytes [{s.start:#x}, {s.stop:#x}) of the slab were never placed")


def test_offsets_and_positions_beyond_4_gib(codec, R, slab):
    """The payload source is the 6.5 GiB slab, of which three blocks of 8 KiB
    are placed: across 2^31, across 2^32 and at 2^32 + 2^31 + 5. Two pieces
    of 2^31 - 1 bytes each, both the slab's first bytes, bring the stream
    position to 2^32 - 2 (nothing of them is gathered but the last bytes of
    the second, which lie in the first block); small pieces with `off` in all
    three blocks follow. The expected bytes come from a control run on the
    device — the same small pieces over the three blocks packed into a 24 KiB
    tensor — and from the model over the sparse slab."""
    rng = np.random.default_rng(91)
    blk = 8192
    bases = [G31 - 3000, G32 - 3000, FAR]
    data = [rng.integers(0, 256, blk, dtype=np.uint8) for _ in bases]
    slab.clear()
    for b, d in zip(bases, data):
        slab.place(b, d)
    marks = rng.integers(0, 256, 64, dtype=np.uint8)
    hdr = rng.integers(0, 256, 500, dtype=np.uint8)
    giant = 0x7FFFFFFF
    tail = 2999                                       # the second giant's bytes inside the first block: [G31 - 3000, G31 - 1)
    small, ctrl = [], [(0, tail, V.PIECE_PAYLOAD)]
    for i in range(260):
        k = i % 5
        if k == 3:
            p = (int(rng.integers(0, 60)), 4, V.PIECE_MARK)
            small.append(p), ctrl.append(p)
        elif k == 4:
            ln = int(rng.integers(1, 120))
            p = (int(rng.integers(0, 500 - ln)), ln, V.PIECE_HDR)
            small.append(p), ctrl.append(p)
        else:
            ln = int(rng.integers(1, 400))
            # across 2^31 / 2^32 every so often, else anywhere in the block
            o = 3000 - ln // 2 if i % 15 == k else int(rng.integers(0, blk - ln))
            small.append((bases[k] + o, ln, V.PIECE_PAYLOAD))
            ctrl.append((k * blk + o, ln, V.PIECE_PAYLOAD))
    far = G.make_pieces([(0, giant, V.PIECE_PAYLOAD), (0, giant, V.PIECE_PAYLOAD)] + small)
    assert ((far["off"] < G31) & (far["off"] + far["len"] > G31) & (far["len"] < 1000)).sum() >= 3
    assert ((far["off"] < G32) & (far["off"] + far["len"] > G32)).sum() >= 3 and (far["off"] > G32 + G31).sum() > 30
    # the control: everything small, on the device
    c = Listed(R, codec, G.make_pieces(ctrl), [marks, hdr, np.concatenate(data)])
    control = c.window(0, c.total).copy()
    assert c.total > 4 * G.TILE
    # the far list
    sparse = Sparse(SLAB, list(zip(bases, data)))
    lst = Listed(R, codec, far, [marks, hdr, sparse], d_sources=[_dev(marks), _dev(hdr), slab.t],
                 lens=[64, 500, SLAB])
    delta = 2 * giant - tail                          # stream position of the control's byte 0
    assert lst.total == delta + c.total and int(lst.pos[2]) == G32 - 2 and int(lst.res[1]) == 0
    for start, count in ((G32 - 5 - 2000, 4096), (G32 - 5, 10), (G32 - 2, 2), (G32 + 8192 - 100, 3000),
                         (G32 + 8192, 8192 + 17), (lst.total - 500, 600)):
        for shift in (0, 13):
            want = np.full(count, SENT, np.uint8)
            k = min(count, lst.total - start)
            want[:k] = control[start - delta:start - delta + k]
            mod = np.full(count, SENT, np.uint8)
            G.gather(far, lst.pos, lst.sources, start, count, mod, lst.lens)
            assert np.array_equal(mod, want), "the model over the sparse slab and the control run disagree"
            lst.window(start, count, shift, want=want)
    slab.check()
    assert BW.relocate_offsets(c.pos[1:], delta).tolist() == lst.pos[2:].tolist()


# ---------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------
def test_graph_capture_and_replay(R):
    import torch
    lists = []
    for seed in (31, 32):
        iov, hdr, pay, _, _ = V.build(V.random_splits(300, seed), seed=seed)
        m = V.fragment_iov(iov, 16)
        lists.append((m["pieces"], [np.frombuffer(m["marks"], np.uint8), np.frombuffer(hdr, np.uint8),
                                    np.frombuffer(pay, np.uint8)]))
    n = max(len(p) for p, _ in lists)
    cap = [max(len(s[k]) for _, s in lists) for k in range(3)]
    total = max(int(p["len"].astype(np.int64).sum()) for p, _ in lists)
    d_pieces = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    d_src = [torch.zeros(c, dtype=torch.uint8, device="cuda") for c in cap]
    src = R.gather_src(*d_src)
    pos = torch.full((n + 1,), -2, dtype=torch.int64, device="cuda")
    res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    out = torch.full((total + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()

    def work(codec):
        codec.piece_offsets(d_pieces, n, src, pos, res)
        codec.gather_pieces(d_pieces, pos, n, src, 0, total, out)

    fresh = R.Codec(0, stream=s.cuda_stream)
    codec = R.Codec(0, stream=s.cuda_stream)
    try:
        err = None
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            try:
                fresh.piece_offsets(d_pieces, n, src, pos, res)
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
        for pieces, sources in lists:
            padded = np.zeros(n, V.PIECE_DTYPE)      # the list padded with empty pieces
            padded[:len(pieces)] = pieces
            d_pieces.copy_(torch.from_numpy(padded.view(np.uint8).copy()))
            for t, a in zip(d_src, sources):
                t[:len(a)] = torch.from_numpy(a.copy())
            out.fill_(SENT)
            g.replay()
            torch.cuda.synchronize()
            want_pos, want_res = G.piece_offsets(padded, cap)
            assert np.array_equal(pos.cpu().numpy().view(np.uint64), want_pos)
            assert res.cpu().numpy().view(np.uint64).tolist() == want_res.tolist()
            k = int(want_res[0])
            got = out.cpu().numpy()
            assert got[:k].tobytes() == G.stream(pieces, sources).tobytes() and (got[k:] == SENT).all()
    finally:
        fresh.close()
        codec.close()


# ---------------------------------------------------------------------------
# 8. the C++ mirror
# ---------------------------------------------------------------------------
def test_cpp_mirror_serialise_fragmented():
    exe = os.path.join(ROOT, "tests", "cpp_gather", "test_gather")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_gather" in r.stdout
