"""tests/big_wire.py (the expected values of the GPU tests above 4 GiB)
against the models and the oracle on real, small concatenations: a moved
wire, and lead | W x 3 | tail with an odd |W| of about 2 KiB."""
import struct

import numpy as np
import pytest

import big_wire as BW
import fragment_encode_model as FE
import fragment_iov_model as FV
import fragment_model as FR
import fragment_streams_model as FS
import frame_model as FM
import heads_model as HM
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
import streams_model as SM
from test_gpu_parity import all_golden_records, assert_decoded_equal

MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
P = 3


def _split(wire, off):
    return [bytes(wire[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def same_decoded(got, want, what):
    assert_decoded_equal(got, want, what)
    n = len(want[2])
    assert np.array_equal(got[1].view(np.uint8)[:192 * n], want[1].view(np.uint8)[:192 * n]), what + ": unix table"


@pytest.fixture(scope="module")
def parts(oracle):
    """(lead, W, tail, W's records): W = 16 mixed records, an AUTH_UNIX call
    at the associated-data limit and a record of a few bytes that makes |W| odd."""
    wire, off, st, _ = oracle.encode_batch(S.mixed(16, seed=5, pmin=0, pmax=160, exotic=0.3))
    assert not st.any()
    recs = _split(wire, off) + [HM.big_unix_call(77, b"\1\2\3\4")[0]]
    recs.append(FM.opaque(b"\0\0\0\5\1\2"[:5 + sum(map(len, recs)) % 2]))
    W = b"".join(recs)
    assert len(W) % 2 == 1 and 1800 < len(W) < 3000, len(W)
    lead = FM.call(9, b"lead" * 3)
    tail = FM.call(10, b"x" * 40)[:-7]
    return lead, W, tail, recs


def test_relocate_decoded_is_the_oracle_on_a_moved_wire(oracle, golden):
    recs, _ = all_golden_records(golden)
    wire, off, st, _ = oracle.encode_batch(S.mixed(150, seed=3, pmin=0, pmax=90, exotic=0.3))
    recs = recs + _split(wire, off) + [HM.big_unix_call(5)[0]]
    w, o = L.records_from_wire(recs)
    o = np.asarray(o, np.uint64)
    for d in (37, 4096 + 2):
        moved = np.concatenate([np.full(d, 0xEE, np.uint8), w])
        for mode in MODES:
            ctrl = oracle.decode_batch(w, o, mode)
            assert (ctrl[2] == 0).sum() > 150 and (ctrl[2] != 0).sum() > 5
            same_decoded(BW.relocate_decoded(ctrl, d), oracle.decode_batch(moved, BW.relocate_offsets(o, d), mode),
                         f"moved by {d} mode {mode}")


def test_tiled_framing_and_decode(oracle, parts):
    lead, W, tail, recs = parts
    stream = lead + W * P + tail
    lo = FE.offsets_of([lead])
    wo = FE.offsets_of(recs)
    off, n, consumed, st, a0, a1 = oracle.frame_stream(stream)
    want = BW.tile_offsets(lo, wo, P)
    assert n == 1 + P * len(recs) and np.array_equal(off, want)
    assert (consumed, st, a0, a1) == (int(want[-1]), FM.INCOMPLETE_MESSAGE, len(tail), len(tail) + 7)
    host = np.frombuffer(stream + b"\0" * 16, np.uint8)
    for mode in MODES:
        dl = oracle.decode_batch(np.frombuffer(lead + b"\0" * 16, np.uint8), lo, mode)
        dw = oracle.decode_batch(np.frombuffer(W + b"\0" * 16, np.uint8), wo, mode)
        assert (dw[2] != 0).any() and (dw[2] == 0).sum() >= 16
        same_decoded(BW.tile_decoded(dl, dw, P, len(lead), len(W)), oracle.decode_batch(host, off, mode),
                     f"tiled decode mode {mode}")


def test_pack_unix_slots_crosses_groups(oracle):
    """More than 64 records per block and a lead: the groups of 64 fall
    differently in every block."""
    wire, off, st, _ = oracle.encode_batch(S.mixed(75, seed=8, pmin=0, pmax=20))
    W = bytes(wire)
    lead = FM.call(1)
    lo, wo = FE.offsets_of([lead]), np.asarray(off, np.uint64)
    host = np.frombuffer(lead + W * P + b"\0" * 16, np.uint8)
    for mode in MODES:
        dl = oracle.decode_batch(np.frombuffer(lead + b"\0" * 16, np.uint8), lo, mode)
        dw = oracle.decode_batch(np.frombuffer(W + b"\0" * 16, np.uint8), wo, mode)
        same_decoded(BW.tile_decoded(dl, dw, P, len(lead), len(W)),
                     oracle.decode_batch(host, BW.tile_offsets(lo, wo, P), mode), f"mode {mode}")


def test_gather_decoded_is_the_oracle_on_each_slice(oracle, golden):
    """Records read from two copies of a wire in any order (the expected
    values of onc_decode_extents), and the probe for the body-level roots."""
    from test_gpu_extents import expect_extents
    recs, _ = all_golden_records(golden)
    wire, off, st, _ = oracle.encode_batch(S.mixed(150, seed=3, pmin=0, pmax=90, exotic=0.3))
    recs = recs + _split(wire, off)
    w, o = L.records_from_wire(recs)
    o = np.asarray(o, np.uint64)
    n, T, d = len(recs), int(o[-1]), int(o[-1]) + 21
    both = np.concatenate([w[:T], np.full(21, 0xEE, np.uint8), w])
    length = np.diff(o.astype(np.int64)).astype(np.uint32)
    rng = np.random.default_rng(2)
    for idx, far in ((np.arange(n)[::-1], np.ones(n, bool)), (np.arange(n), np.arange(n) % 2 == 1),
                     (rng.permutation(n), rng.random(n) < 0.5)):
        delta = np.where(far, d, 0).astype(np.uint64)
        for mode in MODES:
            ctrl = oracle.decode_batch(w, o, mode)
            want = expect_extents(oracle, both, o[:-1][idx] + delta, length[idx], len(both), mode)
            same_decoded(BW.gather_decoded(ctrl, idx, delta), want[:5], f"mode {mode}")
    for mode in MODES:
        ctrl = oracle.decode_batch(w, o, mode)
        moved = oracle.decode_batch(both, o + np.uint64(d), mode)
        same_decoded(BW.relocate_by_probe(ctrl, moved, d, 12345), BW.relocate_decoded(ctrl, 12345), "probe")


def test_relocate_batch_encodes_the_same_wire(oracle):
    hb = S.mixed(120, seed=6, pmin=0, pmax=70, exotic=0.3)
    wire = oracle.encode_batch(hb)[0]
    msgs, unix = BW.relocate_batch(hb, payload=37, auth=11)
    pad = lambda a, k: np.concatenate([np.full(k, 0xEE, np.uint8), a])
    far = L.HostBatch(msgs, unix, pad(hb.auth_arena, 11), pad(hb.payload_arena, 37))
    got, _, st, _ = oracle.encode_batch(far)
    assert not st.any() and got == wire


@pytest.mark.parametrize("F", [1, 100, 160, 1024])
def test_tiled_fragment_frame_defragment_and_heads(parts, F):
    lead, W, tail, recs = parts
    stream = lead + W * P
    lo, wo = FE.offsets_of([lead]), FE.offsets_of(recs)
    off = BW.tile_offsets(lo, wo, P)
    ml, mw, whole = FE.fragment(lead, lo, F), FE.fragment(W, wo, F), FE.fragment(stream, off, F)
    t = BW.tile_fragment(ml, mw, P)
    for k in ("out_off", "status", "result"):
        assert np.array_equal(t[k], whole[k]), k
    fl, fw = FE.stream_bytes(ml), FE.stream_bytes(mw)
    out = FE.stream_bytes(whole)
    assert out == fl + fw * P
    # the receive side of that output
    fo_l, fo_w = FR.frame_fragments(fl)[0], FR.frame_fragments(fw)[0]
    fo, nfrag, consumed, st = FR.frame_fragments(out)[:4]
    assert np.array_equal(fo, BW.tile_offsets(fo_l, fo_w, P)) and (consumed, st) == (len(out), 0)
    assert b"".join(FR.defragment(out, fo)["records"]) == stream
    pend = FR.fragment(b"p" * 50, [10, 30])[:-24]               # two fragments of an unfinished record behind it
    assert np.array_equal(FR.frame_fragments(out + pend)[0],
                          BW.tile_offsets(fo_l, fo_w, P, tail=FR.frame_fragments(pend)[0]))
    for head_len in (160, 736):
        hl = HM.defragment_heads(fl, fo_l[:-1], np.diff(fo_l.astype(np.int64)), head_len)
        hw = HM.defragment_heads(fw, fo_w[:-1], np.diff(fo_w.astype(np.int64)), head_len)
        hh = HM.defragment_heads(out, fo[:-1], np.diff(fo.astype(np.int64)), head_len)
        th = BW.tile_heads(hl, hw, P, len(fo_l) - 1, len(fo_w) - 1)
        for k in ("rec_len", "rec_frag", "frag_pre", "status"):
            assert np.array_equal(th[k], hh[k]), k


def test_relocated_segments(parts):
    """Segments moved inside a slab: rec_start / frag_start move with them,
    the rows' first index follows the order, consumed and aux stay."""
    lead, W, tail, recs = parts
    segs = [lead + W, W + tail, FM.reply28(3) * 20 + b"\x80\0"]
    ctrl = [SM.frame_streams(s, [0], [len(s)]) for s in segs]
    frag = [FE.stream_bytes(FE.fragment(s, FM.true_starts(s)[0].tolist() + [FM.true_starts(s)[1]], 100)) +
            s[FM.true_starts(s)[1]:] for s in segs]
    fctrl = [FS.frame_fragment_streams(s, [0], [len(s)]) for s in frag]
    for order in ((0, 1, 2), (2, 1, 0)):
        for which, ctl, rowlen in ((segs, ctrl, 6), (frag, fctrl, 8)):
            slab = SM.Slab(front=13)
            at = {i: slab.add(which[i], gap=9) for i in (0, 1, 2)}
            buf, off, ln = slab.done()
            so, sl = off[list(order)], ln[list(order)]
            if rowlen == 6:
                m = SM.frame_streams(buf, so, sl)
                start, rows = m.rec_start, m.rows
            else:
                m = FS.frame_fragment_streams(buf, so, sl)
                start, rows = m.frag_start, m.rows
            first, want_start, want_rows = 0, [], []
            first_rec = 0
            for i in order:
                c = ctl[i]
                want_start.append(BW.relocate_offsets(c.rec_start if rowlen == 6 else c.frag_start, off[at[i]]))
                r = BW.relocate_seg_rows(c.rows, first)
                if rowlen == 8:
                    r[:, 6] += np.uint64(first_rec)
                    first_rec += int(c.rows[0, 7])
                want_rows.append(r)
                first += int(c.rows[0, 1])
            assert np.array_equal(start, np.concatenate(want_start)), (order, rowlen)
            assert np.array_equal(rows, np.concatenate(want_rows)), (order, rowlen)


def test_relocated_iov_and_pieces():
    iov, hdr, payload = FV.build(FV.random_splits(40, seed=4), seed=4)[:3]
    ctrl = FV.fragment_iov(iov, 24)
    far = BW.relocate_iov(iov, payload=(1 << 32) + 5, wire=1 << 33, hdr=48)
    m = FV.fragment_iov(far, 24)
    want = BW.relocate_pieces(BW.relocate_pieces(ctrl["pieces"], (1 << 32) + 5), 48, L.PIECE_HDR)
    assert np.array_equal(m["pieces"], want) and m["marks"] == ctrl["marks"]
    for k in ("out_off", "piece_off", "status", "result"):
        assert np.array_equal(m[k], ctrl[k]), k
    assert (far["payload_off"][iov["payload_len"] > 0] > 1 << 32).all()


@pytest.mark.parametrize("length", [4, 5, 1000])
@pytest.mark.parametrize("F", [1, 7, 996, 997])
def test_giant_fragments(length, F):
    rng = np.random.default_rng(length * 1000 + F)
    ext = struct.pack(">I", 0x80000000 | (length - 4)) + rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes()
    m = FE.fragment(ext, [0, length], F)
    out = FE.stream_bytes(m)
    rows = BW.giant_fragments(length, F)
    assert len(rows) == int(m["result"][0])
    pos = 0
    for o, s, ln, mark in rows.tolist():
        assert o == pos and out[o:o + 4] == struct.pack(">I", mark) and out[o + 4:o + 4 + ln] == ext[s:s + ln]
        pos = o + 4 + ln
    assert pos == len(out) == int(m["result"][1])
