"""The decode's window loaders (decode.hip: load_round1, stage_round1,
load_round2_coop, stage_round2) at their edges, bit-exact against the CPU
oracle (descriptors, AUTH_UNIX slots, status, aux0, aux1):

* the per-lane fallback of round 2, taken when records that need a second
  round lie 2 GiB or more apart, next to lanes with 3 and 4 round-1 chunks,
  one and two passes;
* the `near` threshold of both loaders at its last near and first far value;
* the header-extent guess of stage_round1 swept over every credential and
  verifier length, at every record alignment, and cut at every chunk edge;
* waves in which one lane, every lane or only the tail lanes need round 2.

`_plan` restates the standard policy's rule for the chunks each round takes
(decode.hip round1_chunks / stage_round1); it only proves that a batch
reaches the case it was built for — results are always the oracle's."""
import numpy as np
import pytest

import onc_rpc_amd.layout as L
from test_gpu_parity import assert_decoded_equal
from test_gpu_r03 import _same_decode

pytestmark = pytest.mark.gpu

MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
WIN_CHUNKS = 10          # decode.hip kWinChunks
NONE = {"kind": "none", "data": None}


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codec(R):
    """The standard policy pinned: round 2 goes through load_round2_coop."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    c = R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD)
    yield c
    c.close()


@pytest.fixture(scope="module")
def line_codec(R):
    c = R.Codec(0, decode_policy=R.DECODE_POLICY_LINE)
    yield c
    c.close()


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def _bytes(rng, n):
    return rng.bytes(int(n)).hex()


def _unix(rng, name_len, ngids):
    return {"kind": "unix", "stamp": int(rng.integers(0, 2**32)), "machine_name": _bytes(rng, name_len),
            "uid": int(rng.integers(0, 2**32)), "gid": int(rng.integers(0, 2**32)),
            "gids": [int(x) for x in rng.integers(0, 2**32, ngids)]}


def _opaque_auth(rng, kind, n):
    if kind == "none":
        return {"kind": "none", "data": _bytes(rng, n) if n else None}
    if kind == "short":
        return {"kind": "short", "data": _bytes(rng, n)}
    return {"kind": "unknown", "id": int(rng.integers(3, 2**32)), "data": _bytes(rng, n)}


def _call(rng, xid, cred=NONE, verf=NONE, plen=0):
    return {"xid": xid, "type": "call", "program": 100003, "program_version": 4, "procedure": xid & 31, "cred": cred,
            "verf": verf, "payload": _bytes(rng, plen)}


def _reply(rng, xid, verf=NONE, plen=0):
    return {"xid": xid, "type": "reply", "reply": "accepted", "verf": verf, "accept_status": "success",
            "payload": _bytes(rng, plen)}


def _encode(oracle, msgs):
    """Message dicts -> list of record bytes (the oracle's encoding)."""
    wire, off, st, _ = oracle.encode_batch(L.build_batch(msgs))
    assert not st.any()
    return [wire[int(off[i]):int(off[i + 1])] for i in range(len(msgs))]


def _pad4(x):
    return (4 - x % 4) % 4


def _plan(wire, off, ln):
    """(nch, want) of a record of ln bytes at wire offset off (the wire
    16-byte aligned) under the standard policy: round 1 takes nch chunks,
    the header needs want; want > nch is a round 2 of want - nch chunks."""
    if ln == 0:
        return 0, 0

    def be(k):
        return int.from_bytes(bytes(wire[off + k:off + k + 4]), "big")

    q0 = off & 15
    avail = min(WIN_CHUNKS, (q0 + ln + 15) >> 4)
    nch = min(4, (q0 + min(ln, 44) + 15) >> 4, avail)
    need = min(ln, 16 * WIN_CHUNKS)
    if ln >= 36 and 16 * nch >= q0 + 36:
        mt = be(8)
        if mt == 0:
            cl = be(32)
            vpos = 36 + cl + _pad4(cl) + 4
            if cl > 200:
                need = 36
            elif q0 + vpos + 4 <= 16 * nch and vpos + 4 <= ln:
                vl = be(vpos)
                need = vpos + 4 + (vl + _pad4(vl) if vl <= 200 else 0)
            else:
                need = vpos + 4 + 16
        elif mt == 1:
            vl = be(20)
            need = 24 + vl + _pad4(vl) + 12 if vl <= 200 else 24
    return nch, min(avail, (q0 + need + 15) >> 4)


def _plans(wire, off):
    off = [int(x) for x in off]
    return [_plan(wire, off[i], off[i + 1] - off[i]) for i in range(len(off) - 1)]


def _long_header_wave(oracle, rng, n_more=200):
    """Records for lanes 1-63 of a wave and n_more for later waves:
    AUTH_UNIX and long opaque-credential Calls (round 2 after 3 or 4 chunks
    depending on the start offset; headers over 112 bytes: two passes),
    AUTH_NONE Calls and empty records; odd payload lengths move the starts
    over every offset in a granule."""
    msgs, empty = [], set()
    for i in range(63 + n_more):
        k = i % 7
        plen = int(rng.integers(0, 40))
        if k == 0:
            msgs.append(_call(rng, i, _unix(rng, int(rng.integers(0, 17)), 16), NONE, plen))
        elif k == 1:
            msgs.append(_call(rng, i, _opaque_auth(rng, "short", int(rng.integers(100, 201))), NONE, plen))
        elif k == 2:
            msgs.append(_call(rng, i, NONE, NONE, plen))
        elif k == 3:
            msgs.append(_call(rng, i, _unix(rng, 64 + int(rng.integers(0, 60)), 16),
                              _opaque_auth(rng, "unknown", int(rng.integers(0, 60))), plen))
        elif k == 4:
            empty.add(i)
            msgs.append(_call(rng, i))
        elif k == 5:
            msgs.append(_call(rng, i, _opaque_auth(rng, "unknown", int(rng.integers(20, 70))),
                              _opaque_auth(rng, "short", int(rng.integers(0, 30))), plen))
        else:
            msgs.append(_reply(rng, i, _opaque_auth(rng, "short", int(rng.integers(30, 201))), plen))
    recs = _encode(oracle, msgs)
    return [b"" if i in empty else r for i, r in enumerate(recs)]


def _far_batch(oracle, rec1_at, rest, seed):
    """Record 0: an AUTH_UNIX Call with a machine name of 64 bytes or more
    and 16 gids whose mark makes it rec1_at bytes long (its payload: zeros
    up to there); the records `rest` follow from rec1_at on. Returns the
    host wire (lazily zeroed pages), rec_off, and record 0's header bytes."""
    rng = np.random.default_rng(seed)
    h0 = bytearray(_encode(oracle, [_call(rng, 0x1234, _unix(rng, 77, 16), NONE, 0)])[0])
    h0[0:4] = ((rec1_at - 4) | 0x80000000).to_bytes(4, "big")
    tail, toff = L.records_from_wire(rest)
    wire = np.zeros(rec1_at + len(tail) + 16, np.uint8)            # zero pages: not touched
    wire[:len(h0)] = np.frombuffer(bytes(h0), np.uint8)
    wire[rec1_at:rec1_at + len(tail)] = tail
    off = np.concatenate([[0], np.uint64(rec1_at) + toff.astype(np.uint64)]).astype(np.uint64)
    return wire, off, len(h0), len(tail)


def _decode_far(R, c, wire, off, hdr_len, tail_len, mode):
    """The wire built on the device (zeros, then the two populated pieces
    copied in) and decoded there."""
    import torch
    n = len(off) - 1
    rec1_at = int(off[1])
    w = torch.zeros(len(wire), dtype=torch.uint8, device="cuda")
    w[:hdr_len] = torch.from_numpy(wire[:hdr_len].copy()).cuda()
    w[rec1_at:rec1_at + tail_len] = torch.from_numpy(wire[rec1_at:rec1_at + tail_len].copy()).cuda()
    assert w.data_ptr() % 16 == 0
    o = torch.from_numpy(off.view(np.int64).copy()).cuda()
    bufs = R.DecodeBuffers(n)
    c.decode(w, o, n, mode, bufs.msgs, bufs.unix, bufs.status, bufs.aux0, bufs.aux1)
    c.sync()
    got = bufs.to_host()
    del w
    torch.cuda.empty_cache()
    return got


# ---------------------------------------------------------------------------
# (a) round 2's per-lane fallback
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_batch(oracle):
    rng = np.random.default_rng(301)
    big = (1 << 31) - 200
    wire, off, hdr_len, tail_len = _far_batch(oracle, big, _long_header_wave(oracle, rng), 302)
    plans = _plans(wire, off[:65])
    assert plans[0] == (3, WIN_CHUNKS), "record 0 needs the full round 2"
    r2 = [(n, w) for n, w in plans[1:64] if w > n]
    assert len(r2) >= 8
    assert {n for n, _ in r2} == {3, 4}, "round 2 after 3 and after 4 round-1 chunks"
    assert any(w > n + 4 for n, w in r2) and any(w <= n + 4 for n, w in r2), "one pass and two passes"
    assert any(p == (0, 0) for p in plans[1:64]) and any(n and w <= n for n, w in plans[1:64])
    ora = {mode: oracle.decode_batch(wire, off, mode) for mode in MODES}
    for mode in MODES:
        assert ora[mode][2][0] == 0 and int(ora[mode][0]["payload_len"][0]) == big - hdr_len
        slot = ora[mode][1][int(ora[mode][0]["cred_ref"][0])]
        assert (L.kind_of(ora[mode][0]["cred_kind_len"][0]), int(slot["name_len"]), int(slot["ngids"])) == (L.KIND_UNIX, 77, 16)
    yield wire, off, hdr_len, tail_len, ora
    del wire


@pytest.mark.parametrize("mode", MODES)
def test_round2_fallback_far_windows(codec, R, far_batch, mode):
    """Record 0, an AUTH_UNIX Call with a 164-byte header, is 2 GiB - 200
    bytes long: it needs round 2 and so do records of its wave that lie past
    the cooperative loader's 2 GiB resource, so the wave's round 2 takes the
    per-lane path; the later waves take the cooperative one."""
    wire, off, hdr_len, tail_len, ora = far_batch
    got = _decode_far(R, codec, wire, off, hdr_len, tail_len, mode)
    assert_decoded_equal(got, ora[mode], f"far round 2, mode {mode}")
    _same_decode(got, ora[mode], f"far round 2, mode {mode}")


def test_round2_far_windows_line_policy(line_codec, R, far_batch):
    wire, off, hdr_len, tail_len, ora = far_batch
    got = _decode_far(R, line_codec, wire, off, hdr_len, tail_len, L.DECODE_SLICE)
    assert_decoded_equal(got, ora[L.DECODE_SLICE], "far round 2, line policy")


# ---------------------------------------------------------------------------
# (b) the `near` threshold
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [(1 << 31) - 256 - 16, (1 << 31) - 256], ids=["last_near", "first_far"])
def test_near_threshold(codec, R, oracle, dist):
    """Record 1's window lies exactly `dist` above record 0's: the last
    distance one buffer resource covers, and the first it does not. Both
    records need round 2, the other lanes of the wave are empty (a third
    window would itself be far), later waves follow."""
    rng = np.random.default_rng(311)
    rest = _long_header_wave(oracle, rng)
    rest = [rest[3]] + [b""] * 62 + rest[63:]                      # lane 1: a long AUTH_UNIX header
    wire, off, hdr_len, tail_len = _far_batch(oracle, dist + 3, rest, 312)
    plans = _plans(wire, off[:65])
    assert int(off[1]) & ~15 == dist and plans[0] == (3, WIN_CHUNKS)
    assert plans[1][1] > plans[1][0] and plans[1][1] == WIN_CHUNKS, "record 1 needs round 2 up to the window's end"
    assert all(p == (0, 0) for p in plans[2:64])
    ora = oracle.decode_batch(wire, off, L.DECODE_SLICE)
    assert ora[2][0] == 0 and ora[2][1] == 0
    got = _decode_far(R, codec, wire, off, hdr_len, tail_len, L.DECODE_SLICE)
    assert_decoded_equal(got, ora, f"near threshold {dist:#x}")
    del wire


# ---------------------------------------------------------------------------
# (c) header-extent grid
# ---------------------------------------------------------------------------
VERF_LENS = [0, 1, 4, 7, 8, 12, 13, 16, 17, 60, 199, 200]


def _plen(rng, i):
    """Short payloads (the record ends soon after its header) and ones that
    carry the record past the window's 160 bytes, alternating."""
    return int(rng.integers(0, 24)) if i % 2 else int(rng.integers(140, 200))


@pytest.fixture(scope="module")
def grid(oracle):
    """[(record bytes, header length)] in a fixed permutation: Calls with
    opaque credentials of every length 0..200 (short, unknown, none with
    data) and verifiers of VERF_LENS, accepted Replies with verifiers of
    every length 0..200, in a fixed permutation, with an AUTH_NONE Call and
    an empty record after every sixth of them."""
    rng = np.random.default_rng(321)
    msgs = []
    for ki, kind in enumerate(("short", "unknown", "none")):
        for cl in range(0 if kind != "none" else 1, 201):
            vl = VERF_LENS[(cl + 5 * ki) % len(VERF_LENS)]
            vk = ("short", "unknown", "none")[(cl + ki) % 3]
            msgs.append(_call(rng, len(msgs), _opaque_auth(rng, kind, cl), _opaque_auth(rng, vk, vl), _plen(rng, cl)))
    for vl in range(201):
        msgs.append(_reply(rng, len(msgs), _opaque_auth(rng, ("short", "unknown", "none")[vl % 3], vl), _plen(rng, vl)))
    ncore = len(msgs)
    for _ in range(ncore // 6 + 1):
        msgs.append(_call(rng, len(msgs), NONE, NONE, int(rng.integers(0, 24))))
    hb = L.build_batch(msgs)
    recs = _encode(oracle, msgs)
    items = [(r, len(r) - int(hb.msgs["payload_len"][i])) for i, r in enumerate(recs)]
    out = []
    for k, i in enumerate(np.random.default_rng(322).permutation(ncore)):
        out.append(items[i])
        if k % 6 == 0:
            out.append(items[ncore + k // 6])                      # an AUTH_NONE Call
        elif k % 6 == 3:
            out.append((b"", 0))
    return out


def _shifted(recs, shift):
    wire, off = L.records_from_wire(recs)
    return np.concatenate([np.zeros(shift, np.uint8), wire]), off + np.uint64(shift)


def test_header_extent_grid_every_alignment(codec, line_codec, R, oracle, grid):
    recs = [r for r, _ in grid]
    seen = set()
    for shift in range(16):
        w, off = _shifted(recs, shift)
        plans = _plans(w, off)
        for wave in range(0, len(plans) - 63, 64):
            p = plans[wave:wave + 64]
            kinds = {"none": any(n and wt <= n for n, wt in p), "r2_3": any(n == 3 and wt > 3 for n, wt in p),
                     "r2_4": any(n == 4 and wt > 4 for n, wt in p), "one": any(n < wt <= n + 4 for n, wt in p),
                     "two": any(wt > n + 4 for n, wt in p), "empty": (0, 0) in p}
            assert all(kinds.values()), (shift, wave, kinds)
        seen |= {(off_ & 15, n, wt) for (n, wt), off_ in zip(plans, off[:-1].astype(np.int64).tolist())}
        for mode in MODES:
            ora = oracle.decode_batch(w, off, mode)
            assert (ora[2][[len(r) != 0 for r in recs]] == 0).all()
            for c, name in ((codec, "standard"), (line_codec, "line")):
                assert_decoded_equal(R.decode_host_wire(c, w, off, mode), ora, f"grid shift {shift} {name} mode {mode}")
    # every round-2 extent after 3 and after 4 round-1 chunks was reached
    assert {(n, wt) for _, n, wt in seen if wt > n} == {(n, wt) for n in (3, 4) for wt in range(n + 1, WIN_CHUNKS + 1)}


def test_header_extent_grid_decode_lengths(codec, R, oracle, grid):
    import torch
    recs = [r for r, _ in grid]
    w, off = _shifted(recs, 5)
    n = len(recs)
    lens = np.diff(off.astype(np.int64)).astype(np.uint32)
    for mode in MODES:
        bufs = R.DecodeBuffers(n)
        rl = torch.from_numpy(lens.view(np.int32).copy()).cuda()
        goff = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        codec.decode_lengths(R.to_device(w, "cuda"), rl, n, 5, mode, bufs.msgs, bufs.unix, bufs.status, bufs.aux0,
                             bufs.aux1, rec_off=goff)
        codec.sync()
        assert np.array_equal(goff.cpu().numpy().view(np.uint64), off)
        _same_decode(bufs.to_host(), oracle.decode_batch(w, off, mode), f"grid decode_lengths mode {mode}")


@pytest.mark.parametrize("shift", [0, 5, 11, 15])
def test_header_extent_grid_cut_at_chunk_edges(codec, line_codec, R, oracle, grid, shift):
    """Every grid record cut (its mark unchanged) to one byte less than, at
    and one byte more than its header length, and to the lengths ending one
    byte before, at and one byte after each 16-byte chunk edge of its window
    up to 176 bytes: the header-extent guess against records that end
    anywhere inside or just past what it asks for."""
    out, pos = [], shift
    for r, h in grid:
        if not r:
            out.append(r)
            continue
        for k in range(3 + 33):
            q0 = pos & 15
            cut = h - 1 + k if k < 3 else 16 * ((k - 3) // 3 + 1) - q0 + (k - 3) % 3 - 1
            if 0 <= cut <= len(r) and 16 * ((k - 3) // 3 + 1) <= 176:
                out.append(r[:cut])
                pos += cut
    # 36 cuts for a record of 177 bytes or more; a cut past a record's own
    # length is dropped, and half the grid's records are short: about 28k
    print(f"cut grid shift {shift}: {len(out)} records")
    assert len(out) >= 27_000, len(out)
    w, off = _shifted(out, shift)
    for mode in MODES:
        ora = oracle.decode_batch(w, off, mode)
        assert (ora[2] != 0).any() and (ora[2] == 0).any()
        for c, name in ((codec, "standard"), (line_codec, "line")):
            assert_decoded_equal(R.decode_host_wire(c, w, off, mode), ora, f"cut grid shift {shift} {name} mode {mode}")


# ---------------------------------------------------------------------------
# (d) wave shapes
# ---------------------------------------------------------------------------
def _wave_parts(oracle):
    """Records whose length is a multiple of 16 (so a wave built from them
    keeps every start at the shift's offset): `long` needs round 2 up to the
    window's end, `short` is an AUTH_NONE Call."""
    rng = np.random.default_rng(331)
    longs = _encode(oracle, [_call(rng, 1000 + i, _unix(rng, 64 + 4 * (i % 8), 16), NONE, 0) for i in range(64)])
    longs = _encode(oracle, [_call(rng, 1000 + i, _unix(rng, 64 + 4 * (i % 8), 16), NONE, -len(r) % 16)
                             for i, r in enumerate(longs)])
    shorts = _encode(oracle, [_call(rng, 2000 + i, NONE, NONE, 4 + 16 * (i % 3)) for i in range(64)])
    assert all(len(r) % 16 == 0 for r in longs + shorts)
    return longs, shorts


@pytest.mark.parametrize("shape", ["lane0", "lane63", "all_full", "one_among_empty", "tail1", "tail63"])
def test_wave_shapes(codec, R, oracle, shape):
    longs, shorts = _wave_parts(oracle)
    full = [shorts[i] for i in range(64)]
    if shape == "lane0":
        recs = [longs[0]] + shorts[1:] + full
    elif shape == "lane63":
        recs = shorts[:63] + [longs[63]] + full
    elif shape == "all_full":
        recs = list(longs) + full
    elif shape == "one_among_empty":
        recs = [b""] * 37 + [longs[5]] + [b""] * 26 + full
    else:
        tail = 1 if shape == "tail1" else 63
        recs = full + full + longs[:tail]                         # n = 64 * 2 + tail: the tail lanes need round 2
    for shift in (0, 3, 9):
        w, off = _shifted(recs, shift)
        plans = _plans(w, off)
        r2 = [i for i, (n, wt) in enumerate(plans) if wt > n]
        want = {"lane0": [0], "lane63": [63], "all_full": list(range(64)), "one_among_empty": [37],
                "tail1": [128], "tail63": list(range(128, 191))}[shape]
        assert r2 == want, (shape, shift, r2)
        if shape == "all_full" and shift <= 4:
            assert all(plans[i] == (3, WIN_CHUNKS) for i in range(64)), "the full 7-chunk round 2 in every lane"
        if shape == "one_among_empty":
            assert all(plans[i] == (0, 0) for i in range(64) if i != 37)
        for mode in MODES:
            ora = oracle.decode_batch(w, off, mode)
            assert (ora[2][[len(r) != 0 for r in recs]] == 0).all()
            assert_decoded_equal(R.decode_host_wire(codec, w, off, mode), ora, f"wave {shape} shift {shift} mode {mode}")
