"""One stream longer than 2^32 bytes through every kernel that walks a wire:
lead | W x P | tail, built on the device, where W is the oracle's encode of
2000 mixed records (about 3.8 MB, an odd length, so every block lies at
another alignment), P the smallest count that brings the stream to 2^32 + 64
MiB, lead one Call sized so that an AUTH_UNIX record starts at 2^32 - 2, and
tail a record cut short. About 2.3M records, 4.4 GB.

Expected values never come from a 4 GiB loop on the host: the oracle and the
models run on lead, on one block and on tail, and tests/big_wire.py tiles
them in closed form (pinned by tests/test_big_wire_model.py). The wire itself
never leaves the device; tables are compared there too. Bit-exact.

Device memory at peak: the stream, a fragmented copy, a rebuilt copy and the
byte mask of one whole-buffer comparison, about 18 GiB."""
import struct

import numpy as np
import pytest

import big_wire as BW
import fragment_encode_model as FE
import fragment_model as FR
import frame_model as FM
import heads_model as HM
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
import streams_model as SM

pytestmark = pytest.mark.gpu

MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
G32 = 1 << 32
NEED = 24 << 30
SENT = 0xA5
FILL = 0x5A
FUSED = 512 * 4096          # records up to which onc_decode_lengths sums its blocks in the decode launch
TOO_LONG, WRITE_ZERO = 100, 105


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codecs(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    cs = {fs: R.Codec(0, force_scan=fs) for fs in (False, True)}
    yield cs
    for c in cs.values():
        c.close()


def dev(a):
    """A host array's bytes as a device tensor of int64 / int32 / uint8."""
    import torch
    a = np.ascontiguousarray(a)
    view = {8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize] if a.dtype.fields is None else np.uint8
    return torch.from_numpy(a.view(view).reshape(-1).copy()).cuda()


def filled(n, dtype):
    import torch
    size = {torch.int64: 8, torch.int32: 4, torch.uint8: 1}[dtype]
    return torch.full((n * size,), FILL, dtype=torch.uint8, device="cuda").view(dtype)


def kept_fill(t, n):
    import torch
    return bool((t.view(-1)[n:].contiguous().view(torch.uint8) == FILL).all().item())


def words(t):
    return t.cpu().numpy().view(np.uint64).copy()


def same(t, host):
    """A device table's first entries equal a host array, compared on the device."""
    import torch
    want = dev(host)
    return torch.equal(t.view(-1)[:want.numel()], want.view(t.dtype) if want.dtype != t.dtype else want)


class Big:
    pass


@pytest.fixture(scope="module")
def big(oracle):
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < NEED:
        pytest.skip(f"needs {NEED} bytes of free device memory, {free} are free")
    b = Big()
    hb = S.mixed(2000, seed=31, pmin=64, pmax=4096)
    wire, off, st, ln = oracle.encode_batch(hb)
    assert not st.any()
    nw = max(i for i in range(1, hb.n + 1) if int(off[i]) % 2 == 1)       # trimmed to an odd length
    b.hb = L.HostBatch(hb.msgs[:nw].copy(), hb.unix, hb.auth_arena, hb.payload_arena)
    b.nw, b.wo = nw, np.asarray(off[:nw + 1], np.uint64)
    b.W = bytes(wire[:int(off[nw])])
    lw = len(b.W)
    assert lw % 2 == 1 and nw > 1900
    # the record that starts at 2^32 - 2: an AUTH_UNIX call of some block
    b.j = next(i for i in range(nw) if hb.msgs["msg_type"][i] == L.MSG_CALL and
               (hb.msgs["cred_kind_len"][i] >> 24) == L.KIND_UNIX and (G32 - 2 - int(off[i])) % lw >= 44)
    lead_len = (G32 - 2 - int(b.wo[b.j])) % lw
    b.lead = FM.call(0xABCD, bytes(np.random.default_rng(5).integers(0, 256, lead_len - 44, dtype=np.uint8)))
    b.P = -(-(G32 + (64 << 20) - lead_len) // lw)
    b.tail = FM.call(0xDCBA, b"t" * 333)[:-100]
    b.lo = np.array([0, lead_len], np.uint64)
    b.off = BW.tile_offsets(b.lo, b.wo, b.P)
    b.n = len(b.off) - 1
    b.T = int(b.off[-1])                                          # the whole records end here
    b.total = b.T + len(b.tail)
    b.kj = (G32 - 2 - lead_len - int(b.wo[b.j])) // lw           # the block of the straddling record
    b.ij = 1 + b.kj * nw + b.j
    assert int(b.off[b.ij]) == G32 - 2 and b.total >= G32 + (64 << 20) and b.n > FUSED + 64
    assert len({(lead_len + k * lw) % 16 for k in range(b.P)}) == 16
    t = torch.empty(b.total + 64, dtype=torch.uint8, device="cuda")
    t[:lead_len] = dev(np.frombuffer(b.lead, np.uint8))
    b.Wd = dev(np.frombuffer(b.W, np.uint8))
    t[lead_len:b.T].view(b.P, lw).copy_(b.Wd.expand(b.P, lw))
    t[b.T:b.total] = dev(np.frombuffer(b.tail, np.uint8))
    t[b.total:] = SENT
    b.stream = t
    b.d_off = dev(b.off)
    b.expected = {}
    b.oracle = oracle
    yield b
    del t, b.stream, b.Wd, b.d_off
    b.expected.clear()
    torch.cuda.empty_cache()


def control(b, mode):
    """The oracle's decode of lead and of W, each from offset 0."""
    o = b.oracle
    return (o.decode_batch(np.frombuffer(b.lead + b"\0" * 16, np.uint8), b.lo, mode),
            o.decode_batch(np.frombuffer(b.W + b"\0" * 16, np.uint8), b.wo, mode))


def expected_decode(b, mode):
    """The tiled decode of the whole stream, on the device: (msgs, unix,
    status, aux0, aux1, the unix slots in use)."""
    if mode not in b.expected:
        dl, dw = control(b, mode)
        assert (dl[2] == 0).all() and (dw[2] == 0).all()
        m, u, st, a0, a1 = BW.tile_decoded(dl, dw, b.P, len(b.lead), len(b.W))
        cred, verf = L.unix_used(m, st)
        slots = np.concatenate([m["cred_ref"][cred], m["verf_ref"][verf]]).astype(np.int64)
        recs = np.concatenate([np.nonzero(cred)[0], np.nonzero(verf)[0]]).astype(np.int64)
        b.expected[mode] = (dev(m), dev(u), dev(st), dev(a0), dev(a1), dev(slots), dev(recs),
                            dev(cred.astype(np.int64)), dev(verf.astype(np.int64)))
    return b.expected[mode]


class Out:
    """Decode outputs for n records and one more, filled."""

    def __init__(self, R, n):
        import torch
        self.n = n
        self.b = R.DecodeBuffers(n + 1)
        for t in self.args():
            t.view(torch.uint8).fill_(FILL)

    def args(self):
        b = self.b
        return b.msgs, b.unix, b.status, b.aux0, b.aux1


def check_decode(b, out, mode, what, n=None, first=0):
    """The n records from record `first` on (a multiple of 64, so the groups
    of 64 fall as in the whole batch and a slot number is the whole batch's
    minus 2 first): every status and row == the tiled control, and the block
    of the straddling record and the last block == the oracle's decode of
    host copies of those two blocks, row by row."""
    import torch
    n = out.n if n is None else n
    assert first % 64 == 0
    em, eu, es, ea0, ea1, slots, recs, cred, verf = expected_decode(b, mode)
    g = out.b
    assert torch.equal(g.status[:n], es[first:first + n]), what + ": status"
    assert torch.equal(g.aux0[:n], ea0[first:first + n]) and torch.equal(g.aux1[:n], ea1[first:first + n]), what + ": aux"
    rows = em.view(torch.int64).view(-1, 8)[first:first + n].clone()
    rows[:, 5] -= 2 * first * cred[first:first + n]              # cred.ref and verf.ref: words 5 and 7 of a descriptor
    rows[:, 7] -= 2 * first * verf[first:first + n]
    assert torch.equal(g.msgs[:64 * n].view(torch.int64).view(-1, 8), rows), what + ": descriptors"
    idx = slots[(recs >= first) & (recs < first + n)]
    assert torch.equal(g.unix.view(-1, 96)[idx - 2 * first], eu.view(-1, 96)[idx]), what + ": AUTH_UNIX slots"
    assert kept_fill(g.msgs, 64 * n) and kept_fill(g.status, n) and kept_fill(g.aux0, n) and kept_fill(g.unix, 192 * n)
    lw, nw = len(b.W), b.nw
    for k in (b.kj, b.P - 1):
        i0 = 1 + k * nw - first                                   # the block's first record among the outputs
        if i0 < 0 or i0 + nw > n:
            continue
        base = len(b.lead) + k * lw
        block = b.stream[base:base + lw].cpu().numpy()
        ora = b.oracle.decode_batch(np.concatenate([block, np.zeros(16, np.uint8)]), b.wo, mode)
        u0 = 2 * (i0 - i0 % 64)
        msgs = g.msgs[64 * i0:64 * (i0 + nw)].cpu().numpy().view(L.MSG_DTYPE).copy()
        unix = g.unix[96 * u0:96 * 2 * (i0 + nw)].cpu().numpy().view(L.UNIX_DTYPE)
        st = g.status[i0:i0 + nw].cpu().numpy()
        for f, mask in zip(("cred", "verf"), L.unix_used(msgs, st)):
            msgs[f + "_ref"][mask] -= np.uint64(u0)
        gm, gp = L.resolve_unix(msgs, unix, st)
        wm, wp = L.resolve_unix(*BW.relocate_decoded(ora, base)[:3])
        assert np.array_equal(st, ora[2]) and np.array_equal(gp, wp), f"{what}: block {k}"
        bad = np.nonzero((gm.view(np.uint8).reshape(-1, 64) != wm.view(np.uint8).reshape(-1, 64)).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: block {k} record {bad[:5]}: {gm[bad[0]]} vs {wm[bad[0]]}"


# ---------------------------------------------------------------------------
# framing
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("force_scan", [False, True])
def test_frame_stream(codecs, big, force_scan):
    import torch
    b, codec = big, codecs[force_scan]
    cases = [("whole", b.total, b.n + 2, b.n, b.T, (FM.INCOMPLETE_MESSAGE, len(b.tail), len(b.tail) + 100)),
             ("stops at the straddling record", b.total, b.ij, b.ij, G32 - 2, (0, 0, 0)),
             ("stops behind it", b.total, b.ij + 1, b.ij + 1, int(b.off[b.ij + 1]), (0, 0, 0)),
             ("ends on a record boundary", int(b.off[b.n - 7]), b.n + 2, b.n - 7, int(b.off[b.n - 7]), (0, 0, 0))]
    for name, length, cap, n, consumed, rest in cases:
        rec_off = filled(cap + 2, torch.int64)
        res = filled(5, torch.int64)
        codec.frame_stream(b.stream, length, rec_off, cap, res)
        codec.sync()
        r = res.cpu().numpy()
        assert (int(r[0]), int(r[1]), int(r[2]), int(np.uint32(r[3])), int(np.uint32(r[4]))) == (n, consumed) + rest, name
        assert torch.equal(rec_off[:n + 1], b.d_off[:n + 1]) and kept_fill(rec_off, n + 1), name
        del rec_off
    assert b.total > 65536 * 65536                    # at 64 KiB chunks: two entries of the third flag level


def test_frame_streams_one_huge_segment(codecs, big):
    """The stream as one segment (seg_len and consumed above 2^32, the
    second chase writing rec_start above the line) between small ones that
    overlap it."""
    import torch
    b, codec = big, codecs[False]
    lead_len = len(b.lead)
    k = 21
    seg_off = [lead_len, 0, 0, int(b.off[b.n - 5])]
    seg_len = [int(b.wo[k]), b.total, lead_len + 1, b.total - int(b.off[b.n - 5])]
    assert SM.KEEP < k and b.total < 1 << 34
    starts = np.concatenate([b.off[1:1 + k], b.off[:-1], b.off[:1], b.off[b.n - 5:-1]])
    lens = np.concatenate([np.diff(b.off[1:2 + k].astype(np.int64)), np.diff(b.off.astype(np.int64)), [lead_len],
                           np.diff(b.off[b.n - 5:].astype(np.int64))]).astype(np.uint32)
    segs = np.repeat(np.arange(4, dtype=np.uint32), [k, b.n, 1, 5])
    cut = (FM.INCOMPLETE_MESSAGE, len(b.tail), len(b.tail) + 100)
    rows = np.array([(0, k, seg_len[0], 0, 0, 0), (k, b.n, b.T) + cut, (k + b.n, 1, lead_len, FM.INCOMPLETE_HEADER, 0, 0),
                     (k + b.n + 1, 5, b.T - seg_off[3]) + cut], np.uint64)
    n = len(starts)
    start = filled(n + 2, torch.int64)
    rlen = filled(n + 2, torch.int32)
    rseg = filled(n + 2, torch.int32)
    d_rows = filled(6 * 4 + 1, torch.int64)
    res = filled(3, torch.int64)
    codec.frame_streams(b.stream, dev(np.array(seg_off, np.uint64)), dev(np.array(seg_len, np.uint64)), 4, start, rlen,
                        rseg, n + 1, d_rows, res)
    codec.sync()
    assert np.array_equal(words(res), np.array([n, n, 3], np.uint64))
    assert np.array_equal(words(d_rows)[:24].reshape(4, 6), rows)
    assert same(start, starts) and same(rlen, lens) and same(rseg, segs)
    assert kept_fill(start, n) and kept_fill(rlen, n) and kept_fill(rseg, n) and kept_fill(d_rows, 24)


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_decode(codecs, R, big, mode):
    b, codec = big, codecs[False]
    out = Out(R, b.n)
    codec.decode(b.stream, b.d_off, b.n, mode, *out.args())
    codec.sync()
    check_decode(b, out, mode, "onc_decode")
    out = Out(R, b.n)
    codec.decode_bounded(b.stream, b.total, b.d_off, b.n, mode, *out.args())
    codec.sync()
    check_decode(b, out, mode, "onc_decode_bounded, wire_len = the stream")
    out = Out(R, b.n)
    codec.decode_bounded(b.stream, b.T, b.d_off, b.n, mode, *out.args())
    codec.sync()
    check_decode(b, out, mode, "onc_decode_bounded, exact fit")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("side", ["below", "above"])
def test_decode_lengths(codecs, R, big, mode, side):
    """Offsets from the lengths alone: the scan inside the decode passes
    2^32, with the record count just below and above what the decode launch
    sums by itself."""
    import torch
    b, codec = big, codecs[False]
    n = FUSED - 3 if side == "below" else b.n
    first = (b.n - n) // 64 * 64                                  # the shorter run starts later and ends above 2^32 too
    assert int(b.off[first]) < G32 < int(b.off[first + n]) and (n > FUSED) == (side == "above")
    rec_len = dev(np.diff(b.off.astype(np.int64)).astype(np.uint32)[first:first + n])
    out = Out(R, n)
    ro = filled(n + 2, torch.int64)
    codec.decode_lengths(b.stream, rec_len, n, int(b.off[first]), mode, *out.args(), rec_off=ro)
    codec.sync()
    check_decode(b, out, mode, f"onc_decode_lengths n {n}", n, first)
    assert torch.equal(ro[:n + 1], b.d_off[first:first + n + 1]) and kept_fill(ro, n + 1)


# ---------------------------------------------------------------------------
# the send side: fragments, and back
# ---------------------------------------------------------------------------
def fragment_control(b, F):
    """The model on lead and on W, tiled: (lead, W, tiled tables, frag(lead), frag(W))."""
    memo = b.__dict__.setdefault("fragment_controls", {})
    if F not in memo:
        ml, mw = FE.fragment(b.lead, b.lo, F), FE.fragment(b.W, b.wo, F)
        memo[F] = (ml, mw, BW.tile_fragment(ml, mw, b.P), FE.stream_bytes(ml), FE.stream_bytes(mw))
    return memo[F]


def run_fragment(codec, b, F, shift, out_cap=None, extra=64):
    """onc_fragment of the whole records of the stream -> (buffer, where out
    starts in it, out_off, status, result)."""
    import torch
    t = fragment_control(b, F)[2]
    total = int(t["out_off"][-1])
    buf = torch.full((16 + shift + total + extra,), SENT, dtype=torch.uint8, device="cuda")
    lo = (-buf.data_ptr()) % 16 + shift
    out_off = filled(b.n + 2, torch.int64)
    status = filled(b.n + 1, torch.int32)
    res = filled(3, torch.int64)
    codec.fragment(b.stream, b.d_off, b.n, F, buf.data_ptr() + lo, out_off, status, res,
                   out_cap=total if out_cap is None else out_cap)
    codec.sync()
    return buf, lo, out_off, status, res


def check_fragmented(b, F, buf, lo, upto=None):
    """The output bytes == frag(lead) | frag(W) x P, and the sentinel around them."""
    import torch
    ml, mw, t, fl, fw = fragment_control(b, F)
    total = int(t["out_off"][-1])
    assert bool((buf[:lo] == SENT).all()) and bool((buf[lo + total:] == SENT).all())
    assert torch.equal(buf[lo:lo + len(fl)], dev(np.frombuffer(fl, np.uint8)))
    body = buf[lo + len(fl):lo + total].view(b.P, len(fw))
    assert bool((body == dev(np.frombuffer(fw, np.uint8))).all()), f"max_frag {F}"
    return total


@pytest.mark.parametrize("F,shift", [(1024, 0), (1024, 5), (8192, 0)])
def test_fragment(codecs, big, F, shift):
    b, codec = big, codecs[False]
    t = fragment_control(b, F)[2]
    buf, lo, out_off, status, res = run_fragment(codec, b, F, shift)
    check_fragmented(b, F, buf, lo)
    assert same(out_off, t["out_off"]) and kept_fill(out_off, b.n + 1)
    assert same(status, t["status"]) and kept_fill(status, b.n) and not t["status"].any()
    assert np.array_equal(words(res), t["result"])
    assert int(t["result"][0]) >= (4_000_000 if F == 1024 else b.n) and int(t["out_off"][-1]) > b.T


def test_fragment_capacity_cut_above_the_line(codecs, big):
    """out_cap ends inside a record that lies above 2^32: that record and all
    after it are ONC_ENC_WRITE_ZERO and nothing of them is written."""
    import torch
    b, codec = big, codecs[False]
    F = 1024
    ml, mw, t, fl, fw = fragment_control(b, F)
    m = b.n - 3 * b.nw - 17
    at = int(t["out_off"][m])
    assert at > G32 and int(b.off[m]) > G32
    buf, lo, out_off, status, res = run_fragment(codec, b, F, 0, out_cap=at + 10)
    want = np.zeros(b.n, np.int32)
    want[m:] = WRITE_ZERO
    assert same(status, want) and same(out_off, t["out_off"]) and np.array_equal(words(res), t["result"])
    assert bool((buf[lo + at:] == SENT).all()), "bytes past the cut were written"
    k = (m - 1) // b.nw                                          # whole blocks before the cut
    assert torch.equal(buf[lo:lo + len(fl)], dev(np.frombuffer(fl, np.uint8)))
    assert bool((buf[lo + len(fl):lo + len(fl) + k * len(fw)].view(k, len(fw)) == dev(np.frombuffer(fw, np.uint8))).all())
    part = at - len(fl) - k * len(fw)
    assert torch.equal(buf[lo + at - part:lo + at], dev(np.frombuffer(fw[:part], np.uint8)))


@pytest.fixture(scope="module")
def fragged(codecs, big):
    """The stream's records cut at 1 KiB by onc_fragment (test_fragment checks
    that output), with two fragments of an unfinished record behind them."""
    import torch
    b = big
    pend = FR.fragment(b"p" * 50, [10, 30])[:-24]
    buf, lo, out_off, status, res = run_fragment(codecs[False], b, 1024, 0, extra=64 + len(pend))
    total = check_fragmented(b, 1024, buf[:buf.numel() - len(pend)], lo)
    buf[lo + total:lo + total + len(pend)] = dev(np.frombuffer(pend, np.uint8))
    ml, mw, t, fl, fw = fragment_control(b, 1024)
    fo = BW.tile_offsets(FR.frame_fragments(fl)[0], FR.frame_fragments(fw)[0], b.P,
                         tail=FR.frame_fragments(pend)[0])
    yield {"wire": buf[lo:], "len": total + len(pend), "total": total, "frag_off": fo, "nfrag": len(fo) - 1,
           "multi": int(t["result"][2]), "pend": pend}
    del buf
    torch.cuda.empty_cache()


def test_frame_fragments_and_defragment(codecs, big, fragged):
    import torch
    b, codec, f = big, codecs[False], fragged
    nfrag = f["nfrag"]
    frag_off = filled(nfrag + 3, torch.int64)
    res = filled(5, torch.int64)
    codec.frame_fragments(f["wire"], f["len"], frag_off, nfrag + 1, res)
    codec.sync()
    assert np.array_equal(words(res), np.array([nfrag, f["len"], 0, 0, 0], np.uint64))
    assert same(frag_off, f["frag_off"]) and kept_fill(frag_off, nfrag + 1)
    out = torch.full((b.T + 64,), SENT, dtype=torch.uint8, device="cuda")
    rec_off = filled(nfrag + 2, torch.int64)
    status = filled(nfrag + 1, torch.int32)
    res = filled(6, torch.int64)
    try:
        codec.defragment(f["wire"], frag_off, nfrag, out, rec_off, status, res, out_cap=b.T)
        codec.sync()
        assert np.array_equal(words(res), np.array([b.n, f["total"], b.T, 2, 30, f["multi"]], np.uint64))
        assert torch.equal(out[:b.T], b.stream[:b.T]) and bool((out[b.T:] == SENT).all())
        assert torch.equal(rec_off[:b.n + 1], b.d_off) and kept_fill(rec_off, b.n + 1)
        assert not bool(status[:b.n].any()) and kept_fill(status, b.n)
    finally:
        del out
        torch.cuda.empty_cache()


def test_fragment_streams_and_defragment_extents(codecs, big, fragged):
    """The fragment stream as one huge rest between small ones."""
    import torch
    b, codec, f = big, codecs[False], fragged
    ml, mw, t, fl, fw = fragment_control(b, 1024)
    fo, nfrag = f["frag_off"], f["nfrag"]
    nl = len(FR.frame_fragments(fl)[0]) - 1                       # the lead's fragments
    seg_off = [0, 0, f["total"]]
    seg_len = [len(fl), f["len"], len(f["pend"])]
    starts = np.concatenate([fo[:nl], fo[:nfrag - 2]])
    lens = np.concatenate([np.diff(fo[:nl + 1].astype(np.int64)), np.diff(fo[:nfrag - 1].astype(np.int64))]).astype(np.uint32)
    n = len(starts)
    rows = np.array([(0, nl, len(fl), 0, 0, 0, 0, 1), (nl, nfrag - 2, f["total"], 0, 0, 0, 1, b.n),
                     (n, 0, 0, 0, 0, 0, 1 + b.n, 0)], np.uint64)
    start = filled(n + 2, torch.int64)
    flen = filled(n + 2, torch.int32)
    d_rows = filled(8 * 3 + 1, torch.int64)
    res = filled(4, torch.int64)
    codec.frame_fragment_streams(f["wire"], dev(np.array(seg_off, np.uint64)), dev(np.array(seg_len, np.uint64)), 3,
                                 start, flen, None, n + 1, d_rows, res)
    codec.sync()
    assert np.array_equal(words(res), np.array([n, n, 1 + b.n, 0], np.uint64))
    assert np.array_equal(words(d_rows)[:24].reshape(3, 8), rows)
    assert same(start, starts) and same(flen, lens) and kept_fill(start, n) and kept_fill(flen, n)
    lead_len = len(b.lead)
    out = torch.full((lead_len + b.T + 64,), SENT, dtype=torch.uint8, device="cuda")
    rec_off = filled(n + 2, torch.int64)
    status = filled(n + 1, torch.int32)
    res = filled(6, torch.int64)
    try:
        codec.defragment_extents(f["wire"], start, flen, n, out, rec_off, status, res, out_cap=lead_len + b.T)
        codec.sync()
        multi = f["multi"] + int(ml["result"][2])
        assert np.array_equal(words(res), np.array([b.n + 1, n, lead_len + b.T, 0, 0, multi], np.uint64))
        assert torch.equal(out[:lead_len], b.stream[:lead_len]) and torch.equal(out[lead_len:lead_len + b.T], b.stream[:b.T])
        assert bool((out[lead_len + b.T:] == SENT).all())
        assert same(rec_off, np.concatenate([[0], b.off + np.uint64(lead_len)]).astype(np.uint64))
        assert not bool(status[:b.n + 1].any()) and kept_fill(rec_off, b.n + 2) and kept_fill(status, b.n + 1)
    finally:
        del out
        torch.cuda.empty_cache()


@pytest.mark.parametrize("head_len", [160, 736])
def test_heads_of_the_fragment_stream(codecs, R, big, fragged, head_len):
    """onc_defragment_heads over the 4.4M fragments, then onc_decode_heads:
    the tables are the tiled model's, and with heads that hold every header
    (736) the decoded rows are onc_decode's with each record's positions moved
    into its slot."""
    import torch
    b, codec, f = big, codecs[False], fragged
    ml, mw, t, fl, fw = fragment_control(b, 1024)
    fo, nfrag = f["frag_off"], f["nfrag"]
    fol, fow = FR.frame_fragments(fl)[0], FR.frame_fragments(fw)[0]
    hl = HM.defragment_heads(fl, fol[:-1], np.diff(fol.astype(np.int64)), head_len)
    hw = HM.defragment_heads(fw, fow[:-1], np.diff(fow.astype(np.int64)), head_len)
    want = BW.tile_heads(hl, hw, b.P, len(fol) - 1, len(fow) - 1)
    n = b.n
    heads = torch.full(((n + 1) * head_len,), SENT, dtype=torch.uint8, device="cuda")
    rec_len = filled(nfrag + 1, torch.int32)
    rec_frag = filled(nfrag + 2, torch.int64)
    frag_pre = filled(nfrag + 1, torch.int64)
    status = filled(nfrag + 1, torch.int32)
    res = filled(6, torch.int64)
    d_start = dev(fo[:-1])
    d_len = dev(np.diff(fo.astype(np.int64)).astype(np.uint32))
    try:
        codec.defragment_heads(f["wire"], d_start, d_len, nfrag, head_len, heads, n, rec_len, rec_frag, frag_pre, status, res)
        codec.sync()
        assert np.array_equal(words(res), np.array([n, nfrag - 2, n * head_len, 2, 30, f["multi"]], np.uint64))
        assert same(rec_len, want["rec_len"]) and same(rec_frag, want["rec_frag"]) and same(status, want["status"])
        assert same(frag_pre, np.concatenate([want["frag_pre"], [0, 10]]).astype(np.uint64))
        assert kept_fill(rec_len, n) and kept_fill(rec_frag, n + 1) and kept_fill(frag_pre, nfrag) and kept_fill(status, n)
        # the heads: a record's first head_len bytes, straight from the stream
        assert bool((heads[n * head_len:] == SENT).all())
        full = dev((want["rec_len"] >= head_len).astype(np.uint8)).bool()
        idx = torch.nonzero(full).view(-1)
        at = b.d_off[:-1][idx]
        got = heads.view(-1, head_len)[idx]
        for c0 in range(0, head_len, 16):
            cols = torch.arange(c0, c0 + 16, device="cuda")
            assert torch.equal(got[:, c0:c0 + 16], b.stream[at[:, None] + cols[None, :]]), c0
        del got
        if head_len < L.HEAD_SPAN_MAX:
            return
        mode = L.DECODE_SLICE
        out = Out(R, n)
        codec.decode_heads(heads, head_len, rec_len, n, mode, *out.args())
        codec.sync()
        dl, dw = control(b, mode)
        both = tuple(np.concatenate([x, y]) for x, y in zip(dl, dw))
        both = (both[0], np.concatenate([dl[1][:2], dw[1]]), both[2], both[3], both[4])
        for fld, mask in zip(("cred", "verf"), L.unix_used(dw[0], dw[2])):
            both[0][fld + "_ref"][1:][mask] += np.uint64(2)
        idx = np.concatenate([[0], np.tile(np.arange(1, b.nw + 1), b.P)])
        ctrl_off = np.concatenate([[0], b.wo[:-1]]).astype(np.uint64)     # each control decodes from offset 0
        delta = np.arange(n, dtype=np.uint64) * np.uint64(head_len) - ctrl_off[idx]
        m, u, st, a0, a1 = BW.gather_decoded(both, idx, delta)
        g = out.b
        assert same(g.status, st) and same(g.aux0, a0) and same(g.aux1, a1) and same(g.msgs, m)
        cred, verf = L.unix_used(m, st)
        used = dev(np.sort(np.concatenate([m["cred_ref"][cred], m["verf_ref"][verf]]).astype(np.int64)))
        assert torch.equal(g.unix.view(-1, 96)[used], dev(u).view(-1, 96)[used])
    finally:
        del heads
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# one extent longer than 4 GiB
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("F", [0x7FFFFFFF, (1 << 20) + 3])
def test_giant_extent(codecs, big, F):
    """onc_fragment of the whole stream as one extent: the position of
    fragment j of an extent whose output exceeds 4 GiB. Then the receive
    side: one record of 2^31 bytes or more is too long and takes nothing."""
    import torch
    b, codec = big, codecs[False]
    Lx = b.total
    rows = BW.giant_fragments(Lx, F)
    k = len(rows)
    total = Lx - 4 + 4 * k
    assert k == (3 if F == 0x7FFFFFFF else k) and k >= 3 and total > G32
    buf = torch.full((total + 64,), SENT, dtype=torch.uint8, device="cuda")
    out_off = filled(3, torch.int64)
    status = filled(2, torch.int32)
    res = filled(3, torch.int64)
    try:
        codec.fragment(b.stream, dev(np.array([0, Lx], np.uint64)), 1, F, buf, out_off, status, res, out_cap=total)
        codec.sync()
        assert np.array_equal(words(res), np.array([k, total, 1], np.uint64))
        assert np.array_equal(words(out_off)[:2], np.array([0, total], np.uint64)) and kept_fill(out_off, 2)
        assert int(status[0].item()) == 0 and kept_fill(status, 1) and bool((buf[total:] == SENT).all())
        marks = dev(np.frombuffer(b"".join(struct.pack(">I", int(x)) for x in rows[:, 3]), np.uint8)).view(k, 4)
        whole = k - 1                                             # fragments of exactly F bytes
        if whole > 3:
            grid = buf[:whole * (F + 4)].view(whole, F + 4)
            assert torch.equal(grid[:, :4], marks[:whole]), "marks"
            assert bool((grid[:, 4:] == b.stream[4:4 + whole * F].view(whole, F)).all()), "bodies"
            todo = rows[whole:]
        else:
            todo = rows
        for o, s, ln, mark in todo.tolist():
            assert buf[o:o + 4].cpu().numpy().tobytes() == struct.pack(">I", mark), o
            assert torch.equal(buf[o + 4:o + 4 + ln], b.stream[s:s + ln]), o
        # back: k fragments, one record, too long
        frag_off = filled(k + 3, torch.int64)
        fres = filled(5, torch.int64)
        codec.frame_fragments(buf, total, frag_off, k + 1, fres)
        codec.sync()
        assert np.array_equal(words(fres), np.array([k, total, 0, 0, 0], np.uint64))
        assert same(frag_off, np.append(rows[:, 0], total).astype(np.uint64)) and kept_fill(frag_off, k + 1)
        out = torch.full((4096,), SENT, dtype=torch.uint8, device="cuda")
        rec_off = filled(k + 2, torch.int64)
        st = filled(k + 1, torch.int32)
        dres = filled(6, torch.int64)
        codec.defragment(buf, frag_off, k, out, rec_off, st, dres, out_cap=4096)
        codec.sync()
        assert np.array_equal(words(dres), np.array([1, total, 0, 0, 0, 1], np.uint64))
        assert np.array_equal(words(rec_off)[:2], np.zeros(2, np.uint64)) and int(st[0].item()) == TOO_LONG
        assert bool((out == SENT).all()) and kept_fill(rec_off, 2) and kept_fill(st, 1)
    finally:
        del buf
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# encode and compact above the line
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiled_batch(R, big):
    """W's descriptors P times over one payload arena, auth arena and
    AUTH_UNIX table: every block names the same payload_off."""
    b = big
    return R.DeviceBatch(b.P * b.nw, dev(np.tile(b.hb.msgs, b.P)), dev(b.hb.unix), dev(b.hb.auth_arena),
                         dev(b.hb.payload_arena))


@pytest.mark.parametrize("how", ["encode", "force_scan", "plan + emit"])
def test_encode_non_uniform_records(codecs, big, tiled_batch, how):
    import torch
    b, db = big, tiled_batch
    codec = codecs[how == "force_scan"]
    n, size, lead_len = db.n, b.P * len(b.W), len(b.lead)
    out = torch.full((size + 64,), SENT, dtype=torch.uint8, device="cuda")
    rec_off = filled(n + 2, torch.int64)
    status = filled(n + 1, torch.int32)
    try:
        if how == "plan + emit":
            codec.encode_plan(db, status)
            codec.encode_emit(db, out, rec_off, status, out_cap=size)
        else:
            codec.encode(db, out, rec_off, status, out_cap=size)
        codec.sync()
        assert torch.equal(out[:size], b.stream[lead_len:b.T]) and bool((out[size:] == SENT).all())
        assert torch.equal(rec_off[:n + 1], b.d_off[1:] - lead_len) and kept_fill(rec_off, n + 1)
        assert not bool(status[:n].any()) and kept_fill(status, n)
    finally:
        del out
        torch.cuda.empty_cache()


def test_compact_two_records_above_the_line(codecs, big):
    """Two extents above 2^32, a few MiB before the end, dropped: few bytes
    move, every offset is large."""
    import torch
    b, codec = big, codecs[False]
    buf = b.stream[:b.T + 64].clone()
    buf[b.T:] = SENT
    i1, i2 = b.n - 3 * b.nw + 11, b.n - b.nw - 40
    o = b.off.astype(np.int64)
    d1, d2 = int(o[i1 + 1] - o[i1]), int(o[i2 + 1] - o[i2])
    assert int(o[i1]) > G32 and d1 > 0 and d2 > 0 and b.T - int(o[i1]) < 16 << 20
    st = np.zeros(b.n, np.int32)
    st[[i1, i2]] = 101
    rec_off = torch.cat([b.d_off, filled(1, torch.int64)])
    try:
        total = codec.compact(buf, rec_off, dev(st), b.n)
        want = o.copy()
        want[i1 + 1:] -= d1
        want[i2 + 1:] -= d2
        assert total == b.T - d1 - d2 == int(want[-1])
        assert same(rec_off, want.astype(np.uint64)) and kept_fill(rec_off, b.n + 1)
        s = b.stream
        assert torch.equal(buf[:o[i1]], s[:o[i1]])
        assert torch.equal(buf[o[i1]:o[i2] - d1], s[o[i1 + 1]:o[i2]])
        assert torch.equal(buf[o[i2] - d1:total], s[o[i2 + 1]:b.T])
        assert torch.equal(buf[total:b.T], s[total:b.T]) and bool((buf[b.T:] == SENT).all())
    finally:
        del buf
        torch.cuda.empty_cache()
