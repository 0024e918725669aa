"""Every entry point with its inputs placed beyond 2^31 and 2^32 bytes of one
device slab (2^32 + 2^31 + 1 MiB, allocated and never filled): the work is
tiny, the positions are not. A workload of a few tens of KiB is written at
base 0 (the control), with a record's mark straddling 2^31 and 2^32, with an
AUTH_UNIX header straddling 2^32, and at 2^32 + 2^31 + 5; what a call writes
for a far copy must be what the oracle or the model gives for the control,
with every wire position moved by the base (tests/big_wire.py, pinned on the
CPU by tests/test_big_wire_model.py). Bit-exact, both decode modes, both
first-round policies.

A difference of two positions truncated to 32 bits still looks far at 2^31
and looks near at 2^32 + 64: the extents test puts both in one wave.

Guards: outputs carry one entry more than the call may write and keep their
fill there; the slab's bytes 4 KiB either side of every placement keep a
sentinel, and the placed bytes stay what they were."""
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
from test_gpu_bounded import _body_records, check, expected
from test_gpu_iov import reassemble
from test_gpu_parity import all_golden_records

pytestmark = pytest.mark.gpu

MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
POLICIES = ["standard", "line"]
G31, G32 = 1 << 31, 1 << 32
SLAB = G32 + G31 + (1 << 20)
FAR = G32 + G31 + 5
GUARD = 4096
SENT = 0xA5
FILL = 0x5A


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codecs(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pol = {"standard": R.DECODE_POLICY_STANDARD, "line": R.DECODE_POLICY_LINE}
    cs = {p: R.Codec(0, decode_policy=pol[p]) for p in POLICIES}
    yield cs
    for c in cs.values():
        c.close()


class Slab:
    """The device slab and what was written into it."""

    def __init__(self, t):
        self.t = t
        self.placed = []

    def data_ptr(self):
        return self.t.data_ptr()

    def numel(self):
        return SLAB

    def clear(self):
        self.placed = []

    def place(self, base, data):
        """`data` (host bytes) at `base`, the sentinel GUARD bytes either side."""
        import torch
        d = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).cuda()
        lo, hi = max(0, base - GUARD), min(SLAB, base + len(d) + GUARD)
        assert 0 <= base and base + len(d) <= SLAB
        for b, x in self.placed:
            assert hi <= b - GUARD or lo >= b + len(x) + GUARD, "placements too close"
        self.t[lo:hi] = SENT
        self.t[base:base + len(d)] = d
        self.placed.append((base, d))

    def check(self):
        """Nothing in or around a placement was written."""
        import torch
        for base, d in self.placed:
            lo, hi = max(0, base - GUARD), min(SLAB, base + len(d) + GUARD)
            want = torch.full((hi - lo,), SENT, dtype=torch.uint8, device="cuda")
            want[base - lo:base - lo + len(d)] = d
            assert torch.equal(self.t[lo:hi], want), f"slab bytes around {base:#x} changed"


@pytest.fixture(scope="module")
def slab():
    import torch
    free = torch.cuda.mem_get_info()[0]
    need = SLAB + (1 << 30)
    if free < need:
        pytest.skip(f"needs {need} bytes of free device memory, {free} are free")
    t = torch.empty(SLAB, dtype=torch.uint8, device="cuda")
    yield Slab(t)
    del t
    torch.cuda.empty_cache()


def _split(wire, off):
    return [bytes(wire[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


def dev64(a):
    import torch
    return torch.from_numpy(np.append(np.ascontiguousarray(a, np.uint64), np.uint64(0)).view(np.int64).copy()).cuda()


def dev32(a):
    import torch
    return torch.from_numpy(np.append(np.ascontiguousarray(a, np.uint32), np.uint32(0)).view(np.int32).copy()).cuda()


def filled(n, dtype):
    """n entries of the fill pattern (every byte FILL)."""
    import torch
    size = {torch.int64: 8, torch.int32: 4, torch.uint8: 1}[dtype]
    return torch.full((n * size,), FILL, dtype=torch.uint8, device="cuda").view(dtype)


def kept_fill(t, n):
    """Entries from n on still hold the fill."""
    import torch
    return bool((t.view(-1)[n:].contiguous().view(torch.uint8) == FILL).all().item())


class Dec:
    """Decode outputs for n records with one record more, filled."""

    def __init__(self, R, n):
        self.b = R.DecodeBuffers(n + 1)
        import torch
        for t in self.args():
            t.view(torch.uint8).fill_(FILL)
        self.b.n = n
        self.n = n

    def args(self):
        b = self.b
        return b.msgs, b.unix, b.status, b.aux0, b.aux1

    def host(self):
        b, n = self.b, self.n
        assert kept_fill(b.msgs, 64 * n) and kept_fill(b.unix, 192 * n) and kept_fill(b.status, n) and \
            kept_fill(b.aux0, n) and kept_fill(b.aux1, n), "a decode wrote past n"
        return b.to_host()


# ---------------------------------------------------------------------------
# the workloads
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def w0(oracle, golden):
    """The golden vectors (error vectors included), 300 mixed records with
    exotic auths, payloads from 0 bytes on and odd lengths, a few of them
    corrupted, AUTH_UNIX calls at the associated-data limit, a plain call
    last: wire, offsets, the oracle's decode per mode, the bases."""
    recs, _ = all_golden_records(golden)
    wire, off, st, _ = oracle.encode_batch(S.mixed(300, seed=21, pmin=0, pmax=150, exotic=0.3))
    assert not st.any()
    cw, co = S.corrupt(np.frombuffer(wire, np.uint8), off.astype(np.int64), frac=0.03, seed=22)
    recs = recs + _split(cw, co)
    u = len(recs) // 2
    recs[u] = HM.big_unix_call(4001, b"\1\2\3")[0]
    recs[u + 70] = HM.big_unix_call(4002)[0]
    recs.append(FM.call(4003, b"last!"))
    w, o = L.records_from_wire(recs)
    o = np.asarray(o, np.uint64)
    T = int(o[-1])
    w = np.asarray(w, np.uint8)[:T]
    assert 20_000 < T < 100_000
    ora = {m: oracle.decode_batch(w, o, m) for m in MODES}
    st = ora[MODES[0]][2]
    assert (st == 0).sum() > 250 and 5 < (st != 0).sum() and st[u] == 0 and st[-1] == 0
    r1, r2 = u - 40, u + 30
    bases = {"control": 0,
             "mark across 2^31": G31 - (int(o[r1]) + 2),
             "mark across 2^32": G32 - (int(o[r2]) + 2),
             "AUTH_UNIX header across 2^32": G32 - (int(o[u]) + 100),
             "2^32 + 2^31 + 5": FAR}
    assert int(o[u + 1]) - int(o[u]) > 240 and FAR + T < SLAB
    return {"wire": w, "off": o, "len": np.diff(o.astype(np.int64)).astype(np.uint32), "T": T, "oracle": ora,
            "bases": bases, "unix": u, "n": len(recs)}


@pytest.fixture(scope="module")
def wf(oracle):
    """A stream every framer accepts: 300 mixed records, an AUTH_UNIX call at
    the limit, zero-length payloads; (clean, the same with a cut record
    behind it)."""
    wire, off, st, _ = oracle.encode_batch(S.mixed(300, seed=23, pmin=0, pmax=150, exotic=0.3))
    assert not st.any()
    clean = bytes(wire) + HM.big_unix_call(4004, b"\7" * 5)[0] + FM.reply28(4005) + FM.call(4006)
    return clean, clean + FM.call(4007, b"cut" * 9)[:-11]


# ---------------------------------------------------------------------------
# decode family
# ---------------------------------------------------------------------------
def one_short(want):
    m, u, s, a0, a1 = (np.array(x, copy=True) for x in want[:5])
    m[-1] = np.zeros(1, L.MSG_DTYPE)[0]
    s[-1], a0[-1], a1[-1] = L.DEC_BAD_EXTENT, L.EXTENT_END_PAST_WIRE, 0
    return m, u, s, a0, a1


@pytest.mark.parametrize("policy", POLICIES)
def test_decode_family(codecs, R, slab, w0, policy):
    import torch
    codec = codecs[policy]
    n, T, off, lens = w0["n"], w0["T"], w0["off"], w0["len"]
    d_len = dev32(lens)
    for name, base in w0["bases"].items():
        slab.clear()
        slab.place(base, w0["wire"])
        d_off = dev64(BW.relocate_offsets(off, base))
        for mode in MODES:
            want = BW.relocate_decoded(w0["oracle"][mode], base)
            short = one_short(want)
            what = f"{name} mode {mode}"
            d = Dec(R, n)
            codec.decode(slab, d_off, n, mode, *d.args())
            codec.sync()
            check(d.host(), want, "onc_decode " + what)
            for bounded, wire_len, exp in ((False, None, want), (True, SLAB, want), (True, base + T, want),
                                           (True, base + T - 1, short)):
                d = Dec(R, n)
                ro = filled(n + 2, torch.int64)
                if bounded:
                    codec.decode_lengths_bounded(slab, wire_len, d_len, n, base, mode, *d.args(), rec_off=ro)
                else:
                    codec.decode_lengths(slab, d_len, n, base, mode, *d.args(), rec_off=ro)
                codec.sync()
                check(d.host(), exp, f"onc_decode_lengths bounded {bounded} wire_len {wire_len} " + what)
                assert np.array_equal(ro.cpu().numpy().view(np.uint64)[:n + 1], BW.relocate_offsets(off, base)), what
                assert kept_fill(ro, n + 1)
                if bounded:
                    d = Dec(R, n)
                    codec.decode_bounded(slab, wire_len, d_off, n, mode, *d.args())
                    codec.sync()
                    g = d.host()
                    check(g, exp, f"onc_decode_bounded wire_len {wire_len} " + what)
                    if exp is short:
                        assert (g[2][-1], g[3][-1], g[4][-1]) == (106, 2, 0)
        slab.check()


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("root", [L.ROOT_AUTH_UNIX_PARAMS, L.ROOT_OPAQUE])
def test_decode_body(codecs, R, oracle, slab, w0, policy, root):
    import torch
    codec = codecs[policy]
    recs, param = _body_records(oracle, root)
    w, o = L.records_from_wire(recs)
    o = np.asarray(o, np.uint64)
    T, n, d = int(o[-1]), len(recs), 24
    w = np.asarray(w, np.uint8)[:T]
    moved = np.concatenate([np.full(d, 0xEE, np.uint8), w])
    prm = dev32(param)
    bases = [0, G31 - (int(o[20]) + 2), G32 - (int(o[40]) + 2), FAR]
    for base in bases:
        slab.clear()
        slab.place(base, w)
        d_off = dev64(BW.relocate_offsets(o, base))
        for mode in MODES:
            ctrl = expected(oracle, w, o[:-1], o[1:], [0] * n, mode, root, param)
            far = expected(oracle, moved, o[:-1] + np.uint64(d), o[1:] + np.uint64(d), [0] * n, mode, root, param)
            assert (ctrl[2] == 0).all() and np.array_equal(ctrl[5], far[5])
            want = BW.relocate_by_probe(ctrl, far, d, base)
            for wire_len, exp in ((None, want), (SLAB, want), (base + T, want), (base + T - 1, None)):
                short = exp is None
                exp = one_short(want) if short else exp
                dd = Dec(R, n)
                cons = filled(n + 1, torch.int32)
                if wire_len is None:
                    codec.decode_body(root, slab, d_off, n, mode, *dd.args(), param=prm, consumed=cons)
                else:
                    codec.decode_body_bounded(root, slab, wire_len, d_off, n, mode, *dd.args(), param=prm,
                                              consumed=cons)
                codec.sync()
                what = f"root {root} base {base:#x} mode {mode} wire_len {wire_len}"
                check(dd.host(), exp, what)
                c = cons.cpu().numpy().view(np.uint32)[:n]
                assert np.array_equal(c[:-1], ctrl[5][:-1]) and c[-1] == (0 if short else ctrl[5][-1]), what
                assert kept_fill(cons, n), what
        slab.check()


def run_ext(R, codec, slab, start, length, mode, wire_len=SLAB):
    n = len(start)
    d = Dec(R, n)
    codec.decode_extents(slab, wire_len, dev64(start), dev32(length), n, mode, *d.args())
    codec.sync()
    return d.host()


@pytest.mark.parametrize("policy", POLICIES)
def test_decode_extents_orders(codecs, R, slab, w0, policy):
    """Ascending and descending at every base."""
    codec = codecs[policy]
    n, off, lens = w0["n"], w0["off"], w0["len"]
    for name, base in w0["bases"].items():
        slab.clear()
        slab.place(base, w0["wire"])
        for idx in (np.arange(n), np.arange(n)[::-1]):
            start = off[:-1][idx] + np.uint64(base)
            for mode in MODES:
                want = BW.gather_decoded(w0["oracle"][mode], idx, np.uint64(base))
                check(run_ext(R, codec, slab, start, lens[idx], mode), want, f"{name} first {idx[0]} mode {mode}")
        slab.check()


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("far", [G32 + 64, G32 + 77, G31 + 48, FAR])
def test_decode_extents_low_and_far_in_one_wave(codecs, R, slab, w0, policy, far):
    """The copy at 0 and a copy `far` bytes on, read in one call: alternating
    (neighbouring lanes' windows are far + small apart, which a 32-bit
    difference takes for near at 2^32 + 64), one low record last in a wave of
    far ones, and one far record last in a wave of low ones."""
    codec = codecs[policy]
    n, off, lens, u = w0["n"], w0["off"], w0["len"], w0["unix"]
    slab.clear()
    slab.place(0, w0["wire"])
    slab.place(far, w0["wire"])
    i = np.arange(n)
    low_last = np.ones(n, bool)
    low_last[63::64] = False
    cases = {"alternating": i % 2 == 1, "alternating from far": i % 2 == 0, "low record last": low_last,
             "far record last": ~low_last}
    for name, is_far in cases.items():
        for idx in (i, i[::-1], np.roll(i, 63 - u)):          # the last: the long AUTH_UNIX call is lane 63
            delta = np.where(is_far, far, 0).astype(np.uint64)
            start = off[:-1][idx] + delta
            for mode in MODES:
                want = BW.gather_decoded(w0["oracle"][mode], idx, delta)
                check(run_ext(R, codec, slab, start, lens[idx], mode), want,
                      f"{name} far {far:#x} first {idx[0]} mode {mode}")
    slab.check()


# ---------------------------------------------------------------------------
# framing of many buffers
# ---------------------------------------------------------------------------
def seg_bases(ctrl_starts, lengths):
    """Where the segments go: 0, a mark across 2^31 and across 2^32, the odd
    far base, and one ending on the slab's last byte."""
    s = [int(x) for x in ctrl_starts]
    return [0, G31 - (s[len(s) // 3] + 2), G32 - (s[len(s) // 2] + 2), FAR, SLAB - lengths[4]]


def run_streams(R, codec, slab, seg_off, seg_len, cap, fragments=False):
    import torch
    nseg = len(seg_off)
    w = 8 if fragments else 6
    start = filled(cap + 1, torch.int64)
    rlen = filled(cap + 1, torch.int32)
    rseg = filled(cap + 1, torch.int32)
    rows = filled(w * nseg + 1, torch.int64)
    res = filled(4 if fragments else 3, torch.int64)
    fn = codec.frame_fragment_streams if fragments else codec.frame_streams
    fn(slab, dev64(seg_off), dev64(seg_len), nseg, start, rlen, rseg, cap, rows, res)
    codec.sync()
    r = res.cpu().numpy().view(np.uint64).copy()
    n = int(r[0])
    assert n <= cap and kept_fill(start, n) and kept_fill(rlen, n) and kept_fill(rseg, n) and kept_fill(rows, w * nseg)
    return (start.cpu().numpy().view(np.uint64)[:n].copy(), rlen.cpu().numpy().view(np.uint32)[:n].copy(),
            rseg.cpu().numpy().view(np.uint32)[:n].copy(),
            rows.cpu().numpy().view(np.uint64)[:w * nseg].reshape(nseg, w).copy(), r, start, rlen)


def expect_streams(ctrl, which, bases, order, fragments):
    """The model's framing of each segment on its own (ctrl[k], from offset
    0), moved to its base and listed in `order`."""
    starts, lens, segs, rows = [], [], [], []
    first = first_rec = stopped = needed = 0
    for s, i in enumerate(order):
        c = ctrl[which[i]]
        cs, cl = (c.frag_start, c.frag_len) if fragments else (c.rec_start, c.rec_len)
        starts.append(BW.relocate_offsets(cs, bases[i]))
        lens.append(cl)
        segs.append(np.full(len(cs), s, np.uint32))
        r = BW.relocate_seg_rows(c.rows, first)
        if fragments:
            r[:, 6] += np.uint64(first_rec)
            first_rec += int(c.rows[0, 7])
        rows.append(r)
        first += len(cs)
        needed += int(c.result[1])
        stopped += int(c.rows[0, 3] != 0)
    res = [first, needed, first_rec, stopped] if fragments else [first, needed, stopped]
    return (np.concatenate(starts), np.concatenate(lens), np.concatenate(segs), np.concatenate(rows),
            np.array(res, np.uint64))


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_frame_streams(codecs, R, slab, wf, order):
    codec = codecs["standard"]
    ctrl = [SM.frame_streams(b, [0], [len(b)]) for b in wf]
    assert ctrl[0].rows[0, 3] == 0 and ctrl[1].rows[0, 3] == SM.INCOMPLETE_MESSAGE and len(ctrl[0].rec_start) > SM.KEEP
    which = [0, 1, 0, 1, 0]
    bases = seg_bases(ctrl[0].rec_start, [len(wf[k]) for k in which])
    slab.clear()
    for k, b in zip(which, bases):
        slab.place(b, wf[k])
    assert bases[4] + len(wf[0]) == SLAB
    idx = list(range(5)) if order == "ascending" else list(range(5))[::-1]
    want = expect_streams(ctrl, which, bases, idx, False)
    so, sl = [bases[i] for i in idx], [len(wf[which[i]]) for i in idx]
    got = run_streams(R, codec, slab, so, sl, len(want[0]) + 3)
    for g, w, name in zip(got, want, ("rec_start", "rec_len", "rec_seg", "seg_result", "result")):
        assert np.array_equal(g, w), f"{order}: {name}"
    assert (want[0] > G32).sum() > 600 and want[0].max() + want[1][np.argmax(want[0])] == SLAB
    slab.check()
    # and the records these extents name decode as the control's
    dec = run_ext(R, codec, slab, got[0][:64], got[1][:64], L.DECODE_SLICE)
    assert (dec[2] == 0).all()


@pytest.fixture(scope="module")
def fragged(codecs, R, wf):
    """wf cut again at 100 body bytes by onc_fragment (checked against the
    model): (fragment stream of clean, the same with pending fragments and a
    cut one behind it)."""
    clean = wf[0]
    starts, stop = FM.true_starts(clean)[:2]
    off = np.append(starts, stop).astype(np.uint64)
    m = FE.fragment(clean, off, 100)
    out, out_off, st, res = R.fragment_host(codecs["standard"], clean, off, 100)
    assert out == FE.stream_bytes(m) and np.array_equal(out_off, m["out_off"]) and not st.any()
    assert np.array_equal(res, m["result"]) and int(res[2]) > 50
    pending = FR.fragment(b"p" * 50, [10, 30])[:-11]           # two whole fragments, the last one (the record's end) cut
    return out, out + pending


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_frame_fragment_streams_and_reassembly(codecs, R, slab, wf, fragged, order):
    import torch
    codec = codecs["standard"]
    ctrl = [FS.frame_fragment_streams(b, [0], [len(b)]) for b in fragged]
    assert ctrl[0].rows[0, 3] == 0 and ctrl[1].rows[0, 3] != 0
    which = [0, 1, 0, 1, 0]
    bases = seg_bases(ctrl[0].frag_start, [len(fragged[k]) for k in which])
    slab.clear()
    for k, b in zip(which, bases):
        slab.place(b, fragged[k])
    idx = list(range(5)) if order == "ascending" else list(range(5))[::-1]
    want = expect_streams(ctrl, which, bases, idx, True)
    so, sl = [bases[i] for i in idx], [len(fragged[which[i]]) for i in idx]
    got = run_streams(R, codec, slab, so, sl, len(want[0]) + 3, fragments=True)
    for g, w, name in zip(got, want, ("frag_start", "frag_len", "frag_seg", "seg_result", "result")):
        assert np.array_equal(g, w), f"{order}: {name}"
    nfrag = len(want[0])
    assert (want[0] > G32).sum() > 1000 and (want[0] < G31).sum() > 300
    # onc_defragment_extents: low and far fragments in one call; the output does not depend on where they lie
    model = FR.defragment(fragged[0], ctrl[0].frag_start.tolist() + [len(fragged[0])])
    assert b"".join(model["records"]) == wf[0]
    one = len(wf[0])
    nrec = len(model["status"])
    out = torch.full((5 * one + 64,), SENT, dtype=torch.uint8, device="cuda")
    rec_off = filled(nfrag + 2, torch.int64)
    status = filled(nfrag + 1, torch.int32)
    res = filled(6, torch.int64)
    codec.defragment_extents(slab, got[5], got[6], nfrag, out, rec_off, status, res, out_cap=5 * one)
    codec.sync()
    assert np.array_equal(res.cpu().numpy().view(np.uint64),
                          np.array([5 * nrec, nfrag, 5 * one, 0, 0, 5 * int(model["result"][5])], np.uint64))
    h = out.cpu().numpy()
    assert h[:5 * one].tobytes() == wf[0] * 5 and (h[5 * one:] == SENT).all()
    assert np.array_equal(rec_off.cpu().numpy().view(np.uint64)[:5 * nrec + 1],
                          BW.tile_offsets([0], model["rec_off"], 5))
    assert not status.cpu().numpy()[:5 * nrec].any() and kept_fill(rec_off, 5 * nrec + 1) and kept_fill(status, 5 * nrec)
    slab.check()


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("head_len", [160, 736])
def test_heads_from_far_extents(codecs, R, oracle, slab, wf, fragged, policy, head_len):
    """onc_defragment_heads over fragments at 0 and far in one call, then
    onc_decode_heads: everything but the positions is the compact model's,
    and rec_frag / frag_pre with the far frag_start find the far bytes."""
    import torch
    codec = codecs[policy]
    fw = fragged[0]
    fo = FR.frame_fragments(fw)[0]
    flen = np.diff(fo.astype(np.int64)).astype(np.uint32)
    nf = len(flen)
    bases = seg_bases(fo[:-1], [len(fw)] * 5)
    slab.clear()
    for b in bases:
        slab.place(b, fw)
    order = [3, 0, 2, 4, 1]
    fs = np.concatenate([BW.relocate_offsets(fo[:-1], bases[i]) for i in order])
    fl = np.tile(flen, 5)
    one = HM.defragment_heads(fw, fo[:-1], flen, head_len)
    nrec = len(one["status"])
    want = BW.tile_heads({"rec_len": one["rec_len"][:0], "rec_frag": one["rec_frag"][:1], "frag_pre": one["frag_pre"][:0],
                          "status": one["status"][:0]}, one, 5, 0, nf)
    n, nfrag = 5 * nrec, 5 * nf
    heads = torch.full(((n + 1) * head_len,), SENT, dtype=torch.uint8, device="cuda")
    rec_len = filled(n + 1, torch.int32)
    rec_frag = filled(n + 2, torch.int64)
    frag_pre = filled(nfrag + 1, torch.int64)
    status = filled(n + 1, torch.int32)
    res = filled(6, torch.int64)
    codec.defragment_heads(slab, dev64(fs), dev32(fl), nfrag, head_len, heads, n, rec_len, rec_frag, frag_pre, status,
                           res)
    codec.sync()
    assert np.array_equal(res.cpu().numpy().view(np.uint64),
                          np.array([n, nfrag, n * head_len, 0, 0, 5 * int(one["result"][5])], np.uint64))
    got = {"rec_len": rec_len.cpu().numpy().view(np.uint32)[:n], "rec_frag": rec_frag.cpu().numpy().view(np.uint64)[:n + 1],
           "frag_pre": frag_pre.cpu().numpy().view(np.uint64)[:nfrag], "status": status.cpu().numpy()[:n]}
    for k in got:
        assert np.array_equal(got[k], want[k]), k
    assert kept_fill(rec_len, n) and kept_fill(rec_frag, n + 1) and kept_fill(frag_pre, nfrag) and kept_fill(status, n)
    exp = HM.expected_heads(one, head_len, nrec * head_len, SENT)
    h = heads.cpu().numpy()
    assert np.array_equal(h[:n * head_len], np.tile(exp, 5)) and (h[n * head_len:] == SENT).all()
    # the locator, with the far positions: a record's last bytes are where it says
    recs = FR.defragment(fw, fo)["records"]
    for r in (0, nrec // 2, nrec - 1, nrec, 3 * nrec + nrec // 3, n - 1):
        rec = recs[r % nrec]
        p = len(rec) - 1
        if p < 4:
            continue
        at = HM.locate(got, fs, r, p)
        assert at >= bases[order[r // nrec]] and int(slab.t[at].item()) == rec[p], r
    # decode from the heads: offsets are relative to the heads, so a block is the control's moved by its slots
    for mode in MODES:
        d = Dec(R, n)
        codec.decode_heads(heads, head_len, rec_len, n, mode, *d.args())
        codec.sync()
        HM.check_decode(d.host(), HM.decode_heads(oracle, recs * 5, head_len, mode), f"head_len {head_len} mode {mode}")
    slab.check()


def test_defragment_far_frag_off(codecs, R, slab, wf, fragged):
    import torch
    codec = codecs["standard"]
    for k, fw in enumerate(fragged):
        fo = FR.frame_fragments(fw)[0]
        nfrag = len(fo) - 1
        model = FR.defragment(fw, fo)
        nrec, total = len(model["status"]), int(model["rec_off"][-1])
        for base in seg_bases(fo[:-1], [len(fw)] * 5):
            slab.clear()
            slab.place(base, fw)
            out = torch.full((total + 64,), SENT, dtype=torch.uint8, device="cuda")
            rec_off = filled(nfrag + 2, torch.int64)
            status = filled(nfrag + 1, torch.int32)
            res = filled(6, torch.int64)
            codec.defragment(slab, dev64(BW.relocate_offsets(fo, base)), nfrag, out, rec_off, status, res, out_cap=total)
            codec.sync()
            wres = model["result"].copy()
            wres[1] += np.uint64(base)                         # wire_consumed is a position
            assert np.array_equal(res.cpu().numpy().view(np.uint64), wres), (k, base)
            assert np.array_equal(out.cpu().numpy(), FR.expected_out(model, total + 64, SENT)), (k, base)
            assert np.array_equal(rec_off.cpu().numpy().view(np.uint64)[:nrec + 1], model["rec_off"])
            assert not status.cpu().numpy()[:nrec].any() and kept_fill(rec_off, nrec + 1) and kept_fill(status, nrec)
            slab.check()
    assert int(wres[3]) > 0                                    # the second stream ends in pending fragments


# ---------------------------------------------------------------------------
# send side
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_frag", [100, 1024])
def test_fragment_far_rec_off(codecs, R, slab, wf, max_frag):
    import torch
    codec = codecs["standard"]
    clean = wf[0]
    starts, stop = FM.true_starts(clean)[:2]
    off = np.append(starts, stop).astype(np.uint64)
    n = len(starts)
    m = FE.fragment(clean, off, max_frag)
    total = int(m["out_off"][-1])
    for base in seg_bases(starts, [len(clean)] * 5):
        slab.clear()
        slab.place(base, clean)
        for shift in (0, 5):
            buf, lo = R.aligned_bytes(total + 64 + shift, SENT)
            out_off = filled(n + 2, torch.int64)
            status = filled(n + 1, torch.int32)
            res = filled(3, torch.int64)
            codec.fragment(slab, dev64(BW.relocate_offsets(off, base)), n, max_frag, buf.data_ptr() + lo + shift,
                           out_off, status, res, out_cap=total)
            codec.sync()
            h = buf.cpu().numpy()
            assert np.array_equal(h[lo + shift:lo + shift + total + 64], FE.expected_out(m, total + 64, SENT)), base
            assert (h[:lo + shift] == SENT).all()
            assert np.array_equal(out_off.cpu().numpy().view(np.uint64)[:n + 1], m["out_off"])
            assert np.array_equal(res.cpu().numpy().view(np.uint64), m["result"])
            assert not status.cpu().numpy()[:n].any() and kept_fill(out_off, n + 1) and kept_fill(status, n)
        slab.check()


@pytest.fixture(scope="module")
def batch(oracle):
    hb = S.mixed(300, seed=25, pmin=0, pmax=150, exotic=0.3)
    wire, off, st, ln = oracle.encode_batch(hb)
    assert not st.any()
    return hb, bytes(wire), off, ln


ARENAS = [(0, 1 << 20), (G31 - 1001, G32 - 2003), (G32 - 777, G31 - 555), (FAR, G32 + 4099), (G32 + 64, FAR)]


@pytest.mark.parametrize("payload_at,auth_at", ARENAS)
def test_encode_from_far_arenas(codecs, R, slab, batch, payload_at, auth_at):
    """Payload arena and auth arena both the slab, declared at its length:
    payload_off, opaque refs and name_off are far and some slices straddle
    2^31 / 2^32. onc_encode, onc_encode_lengths, onc_encode_plan + emit,
    onc_encode_iov, onc_compact_iov and onc_fragment_iov on that list."""
    import torch
    codec = codecs["standard"]
    hb, wire, off, ln = batch
    n = hb.n
    slab.clear()
    slab.place(payload_at, hb.payload_arena)
    slab.place(auth_at, hb.auth_arena)
    assert len(hb.payload_arena) > 1001 and len(hb.auth_arena) > 2003          # the slices at G - 1001 etc. straddle
    msgs, unix = BW.relocate_batch(hb, payload=payload_at, auth=auth_at)
    db = R.DeviceBatch(n, R.to_device(msgs, "cuda"), R.to_device(unix, "cuda"), slab.t, slab.t, auth_len=SLAB,
                       payload_len=SLAB)
    rec_len = filled(n + 1, torch.int32)
    status = filled(n + 1, torch.int32)
    codec.encode_lengths(db, rec_len, status)
    codec.sync()
    assert np.array_equal(rec_len.cpu().numpy().view(np.uint32)[:n], ln) and not status.cpu().numpy()[:n].any()
    assert kept_fill(rec_len, n) and kept_fill(status, n)
    want = np.frombuffer(wire, np.uint8)
    for two_phase in (False, True):
        out = torch.full((len(wire) + 64,), SENT, dtype=torch.uint8, device="cuda")
        rec_off = filled(n + 2, torch.int64)
        status = filled(n + 1, torch.int32)
        if two_phase:
            codec.encode_plan(db, status)
            codec.encode_emit(db, out, rec_off, status, out_cap=len(wire))
        else:
            codec.encode(db, out, rec_off, status, out_cap=len(wire))
        codec.sync()
        h = out.cpu().numpy()
        assert np.array_equal(h[:len(wire)], want) and (h[len(wire):] == SENT).all(), two_phase
        assert np.array_equal(rec_off.cpu().numpy().view(np.uint64)[:n + 1], off)
        assert not status.cpu().numpy()[:n].any() and kept_fill(rec_off, n + 1) and kept_fill(status, n)
    # vectored: the control is the same batch with its arenas at 0 in small tensors
    def iov_of(b, cap):
        hdr = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
        iov = torch.full(((n + 1) * 32,), FILL, dtype=torch.uint8, device="cuda")
        st = filled(n + 1, torch.int32)
        tot = filled(2, torch.int64)
        codec.encode_iov(b, hdr, iov, st, tot, hdr_cap=cap)
        codec.sync()
        assert kept_fill(iov, 32 * n) and kept_fill(st, n) and not st.cpu().numpy()[:n].any()
        return hdr, iov, st, tot.cpu().numpy().view(np.uint64).copy()
    c_hdr, c_iov, _, c_tot = iov_of(R.DeviceBatch.from_host(hb), len(wire))
    ci = c_iov.cpu().numpy()[:32 * n].view(L.IOV_DTYPE)
    hdr_host = c_hdr.cpu().numpy()
    assert reassemble(hb, hdr_host, ci, np.zeros(n, np.int32))[0].tobytes() == wire
    assert np.array_equal(ci["wire_off"], off[:-1]) and int(c_tot[1]) == len(wire)
    assert np.array_equal(ci["payload_off"], hb.msgs["payload_off"])
    f_hdr, f_iov, f_st, f_tot = iov_of(db, len(wire))
    fi = f_iov.cpu().numpy()[:32 * n].view(L.IOV_DTYPE).copy()
    e = BW.relocate_iov(ci, payload=payload_at)
    empty = ci["payload_len"] == 0
    e["payload_off"][empty] = msgs["payload_off"][empty]         # an empty slice: the descriptor's offset as it is
    assert np.array_equal(fi, e), "iov"
    assert torch.equal(f_hdr, c_hdr) and np.array_equal(f_tot, c_tot)
    # onc_fragment_iov reads entries only: its pieces are the control's, the payload ones moved
    got = R.fragment_iov_host(codec, fi, 100)
    model = FV.fragment_iov(ci, 100)
    assert np.array_equal(got[1], BW.relocate_pieces(model["pieces"], payload_at)) and got[0].tobytes() == model["marks"]
    for g, k in zip(got[2:], ("out_off", "piece_off", "status", "result")):
        assert np.array_equal(g, model[k]), k
    frag = FE.fragment(wire, off, 100)
    assert FV.gather(model["pieces"], model["marks"], hdr_host, hb.payload_arena) == FE.stream_bytes(frag)
    # onc_compact_iov with a few records dropped: wire_off placed again, the far payload_off kept
    drop = np.zeros(n, np.int32)
    drop[[3, 64, 65, n - 1]] = 101
    tot = filled(2, torch.int64)
    codec.compact_iov(f_iov, dev32(drop.view(np.uint32)), n, tot)
    codec.sync()
    keep = drop == 0
    e = fi.copy()
    e["hdr_len"][~keep] = 0
    e["payload_len"][~keep] = 0
    kept_len = np.where(keep, ln, 0).astype(np.uint64)
    e["wire_off"] = np.cumsum(kept_len) - kept_len
    assert np.array_equal(f_iov.cpu().numpy()[:32 * n].view(L.IOV_DTYPE), e) and kept_fill(f_iov, 32 * n)
    assert np.array_equal(tot.cpu().numpy().view(np.uint64),
                          np.array([int(e["hdr_len"].sum()), int(kept_len.sum())], np.uint64))
    slab.check()


@pytest.mark.parametrize("limit", [0x7FFFFFFF, 1 << 30, 1 << 20])
def test_fragment_iov_nominal_giants(codecs, R, limit):
    """Entries that name 4 GiB payloads (nothing is read behind an entry):
    the 64-bit piece arithmetic, against the model."""
    codec = codecs["standard"]
    iov = np.zeros(9, FV.IOV_DTYPE)
    hdr = [736, 4, 44, 0, 736, 5, 460, 4, 736]
    pay = [0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0xFFFFFFFE, 0xFFFFFFFF, 1 << 31, 1, 0xFFFFFFFF]
    for i, (h, p) in enumerate(zip(hdr, pay)):
        iov[i] = (1000 * i, (1 << 33) + (i << 34) + 7 * i, (1 << 33) + (i << 33), h, p)
    lim = np.array([limit, limit, 7, limit, 0x7FFFFFFF, limit, 1 << 30, limit, limit], np.uint32)
    for rec_max in (None, lim):
        model = FV.fragment_iov(iov, limit, rec_max_frag=rec_max)
        assert int(model["result"][1]) > 1 << 34 and not model["status"].any()
        if limit == 1 << 20:
            assert int(model["piece_off"][6]) - int(model["piece_off"][5]) == 8193
        marks, pieces, out_off, piece_off, status, res = R.fragment_iov_host(codec, iov, limit, rec_max_frag=rec_max)
        assert np.array_equal(res, model["result"]) and np.array_equal(status, model["status"])
        assert np.array_equal(out_off, model["out_off"]) and np.array_equal(piece_off, model["piece_off"])
        assert np.array_equal(pieces, model["pieces"]) and marks.tobytes() == model["marks"]
        assert int(pieces["off"].max()) > 1 << 37
