"""The zero-copy receive of fragmented records on the GPU:
onc_defragment_heads (defrag_heads.hip) and onc_decode_heads (decode.hip, the
heads form) against their host model (tests/heads_model.py, itself checked on
the CPU in tests/test_heads_model.py), against the library's own packed
reassembly, and end to end against the oracle's decode of the original
unfragmented records. Every comparison is bit-exact, and every output is
pre-filled with sentinels: a stray write fails by comparison.

Between fragments the wires hold bytes that read as record marks. No extent
list points outside its buffer.

The issue's head-boundary case names an AUTH_UNIX Call with 16 gids and a
255-byte name. Such a credential declares 340 bytes and the reference refuses
it at the length word (flavor.rs:83: more than 200), so it cannot decode OK at
any head_len; the boundary is tested with the longest credential that does —
16 gids and a 116-byte name, 200 bytes — and the 255-byte one is tested for
what it gives, InvalidLength at every head_len."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fragment_model as FR
import fragment_streams_model as FS
import heads_model as HM
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
import streams_model as SM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
HEADS = [64, 160, 736]
U64, U32 = np.uint64(2**64 - 1), 0xFFFFFFFF
SENT = 0xA5
INVALID_MESSAGE_TYPE, INVALID_LENGTH, INVALID_RPC_VERSION = 4, 10, 11


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codecs(R):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    cs = {"standard": R.Codec(0, decode_policy=R.DECODE_POLICY_STANDARD),
          "line": R.Codec(0, decode_policy=R.DECODE_POLICY_LINE)}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def codec(codecs):
    return codecs["standard"]


# ---------------------------------------------------------------------------
# 1. the gather against the model
# ---------------------------------------------------------------------------
def _check_heads(R, codec, wire, start, flen, head_len, max_records=None, what=""):
    """onc_defragment_heads == the model: every output array, with what lies
    past the written part still the sentinel. Returns (model, outputs)."""
    nfrag = len(start)
    m = HM.defragment_heads(wire, start, flen, head_len, max_records)
    g = R.defragment_host_heads(codec, wire, start, flen, head_len, max_records=max_records, fill=SENT)
    n = int(m["result"][0])
    assert g["result"].tolist() == m["result"].tolist(), f"{what}: result {g['result']} != {m['result']}"
    raw = g["raw"]
    assert np.array_equal(raw["rec_len"][:n], m["rec_len"]), f"{what}: rec_len"
    assert (raw["rec_len"][n:] == U32).all(), f"{what}: rec_len written from n_records on"
    assert np.array_equal(raw["status"][:n], m["status"]), f"{what}: status"
    assert (raw["status"][n:] == -1).all(), f"{what}: status written from n_records on"
    assert np.array_equal(raw["rec_frag"][:n + 1], m["rec_frag"]), f"{what}: rec_frag"
    assert (raw["rec_frag"][n + 1:] == U64).all(), f"{what}: rec_frag written past n_records"
    assert np.array_equal(raw["frag_pre"][:nfrag], m["frag_pre"]), f"{what}: frag_pre"
    assert (raw["frag_pre"][nfrag:] == U64).all()
    want = HM.expected_heads(m, head_len, len(raw["heads"]), SENT)
    bad = np.nonzero(raw["heads"] != want)[0]
    assert len(bad) == 0, (f"{what}: heads differ first at byte {bad[0] % head_len} of slot {bad[0] // head_len}: "
                           f"{raw['heads'][bad[:8]]} vs {want[bad[:8]]}")
    return m, g


BODIES = (0, 1, 2, 3, 5, 40)


def _mixed_record(rng, nfrag):
    lens = rng.choice(BODIES, nfrag)
    return FR.fragment(rng.bytes(int(lens.sum())), np.cumsum(lens)[:-1].tolist())


def _gather_stream(head_len):
    """About 700 fragments in about 150 records — across the plan's
    256-fragment blocks and the decode's 64-record tiles — with bodies of 0, 1,
    2, 3, 5 and 40 bytes mixed; records of B = 0, head_len - 5, - 4 and - 3
    body bytes, whole and cut; one record whose head lies behind 200 empty
    fragments in 1-byte fragments; a pending run at the end."""
    rng = np.random.default_rng(100 + head_len)
    recs = []
    for i in range(140):
        recs.append(_mixed_record(rng, 40 if i % 35 == 7 else int(rng.integers(1, 7))))
    for B in (0, head_len - 5, head_len - 4, head_len - 3):
        body = rng.bytes(B)
        recs.insert(int(rng.integers(0, len(recs))), FR.fragment(body, []))
        if B:
            cuts = sorted(rng.integers(0, B + 1, 3).tolist())
            recs.insert(int(rng.integers(0, len(recs))), FR.fragment(body, cuts))
    deep = FS.CONT0 * 200 + b"".join(FR._BE.pack(1) + rng.bytes(1) for _ in range(head_len + 40)) + \
        FR._BE.pack(FR.LAST | 50) + rng.bytes(50)
    recs.insert(60, deep)
    return b"".join(recs) + FS._pending(rng, 3), len(recs)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
@pytest.mark.parametrize("head_len", HEADS)
def test_gather_against_the_model_and_the_packed_form(R, codec, head_len, order):
    stream, nrec = _gather_stream(head_len)
    wire, start, flen = FS.scatter(stream, order, seed=53 + head_len)
    assert 600 <= len(start) - (240 + head_len) <= 900 and 145 <= nrec <= 155
    m, g = _check_heads(R, codec, wire, start, flen, head_len, what=f"{order} {head_len}")
    assert int(m["result"][0]) == nrec and int(m["result"][3]) == 3 and int(m["result"][5]) > 100
    assert {0, head_len - 5, head_len - 4, head_len - 3} <= set((m["rec_len"].astype(np.int64) - 4).tolist())
    # against the library itself: slot r is the prefix of record r of the packed reassembly
    out, rec_off, status, res = R.defragment_host_extents(codec, wire, start, flen)
    assert not status.any() and res[[0, 1, 3, 4, 5]].tolist() == g["result"][[0, 1, 3, 4, 5]].tolist()
    assert np.array_equal(g["rec_len"], np.diff(rec_off.astype(np.int64)))
    for r in range(nrec):
        p = min(int(g["rec_len"][r]), head_len)
        a = int(rec_off[r])
        assert g["heads"][r * head_len:r * head_len + p].tobytes() == out[a:a + p], r


@pytest.mark.parametrize("head_len", HEADS)
def test_gather_capacity_is_cut_by_record_index(R, codec, head_len):
    stream, nrec = _gather_stream(head_len)
    wire, start, flen = FS.scatter(stream, "shuffled", seed=7)
    for cap in (0, 1, nrec - 1, nrec):
        m, _ = _check_heads(R, codec, wire, start, flen, head_len, max_records=cap, what=f"max_records {cap}")
        assert m["status"].tolist() == [0] * cap + [HM.ENC_WRITE_ZERO] * (nrec - cap)
        assert int(m["result"][2]) == nrec * head_len


def test_gather_pending_only_and_nothing(R, codec):
    rng = np.random.default_rng(5)
    wire, start, flen = FS.scatter(FS._pending(rng, 4), "descending")
    m, _ = _check_heads(R, codec, wire, start, flen, 64, what="pending only")
    assert m["result"][[0, 1, 2, 3, 5]].tolist() == [0, 0, 0, 4, 0]
    _check_heads(R, codec, wire, start[:0], flen[:0], 160, what="no fragments")


# ---------------------------------------------------------------------------
# 2. the heads decode against the model
# ---------------------------------------------------------------------------
def _decode(R, codec, oracle, recs, head_len, mode, what, exact=None, fill=0, allow_either=False):
    heads, rec_len = HM.heads_of(recs, head_len, fill)
    got = R.decode_host_heads(codec, heads, head_len, rec_len, mode)
    want = HM.decode_heads(oracle, recs, head_len, mode)
    stated = set(exact or {})
    assert set(np.nonzero(want[5])[0].tolist()) <= stated or allow_either, \
        f"{what}: either-or records {np.nonzero(want[5])[0]} without a stated outcome"
    HM.check_decode(got, want, what, exact)
    return got, want


def _golden_records(golden):
    from test_gpu_parity import all_golden_records
    recs, names = all_golden_records(golden)
    return recs, [v["name"] for _, v in names]


@pytest.mark.parametrize("policy", ["standard", "line"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("head_len", [160, 736])
def test_golden_vectors_in_slots(R, codecs, oracle, golden, head_len, mode, policy):
    recs, names = _golden_records(golden)
    codec = codecs[policy]
    # the one error vector longer than 160 bytes fails at its credential length word (byte 32)
    exact = {names.index("unix_len_over_200"): (INVALID_LENGTH, 0, 0)}
    got, want = _decode(R, codec, oracle, recs, head_len, mode, f"golden {head_len} {mode} {policy}", exact)
    # against onc_decode of the packed records: the same up to the offset rebase
    wire, off = L.records_from_wire(recs)
    lm, lu, ls, la0, la1 = R.decode_host_wire(codec, np.append(wire, np.zeros(16, np.uint8)), off, mode)
    gm, gu, gs, ga0, ga1 = got
    same = gs != HM.DEC_BAD_EXTENT
    assert np.array_equal(gs[same], ls[same]) and np.array_equal(ga0[same], la0[same]) and \
        np.array_equal(ga1[same], la1[same])
    if head_len == 736:
        assert same.all()
    ok = gs == 0
    for f in ("xid", "msg_type", "reply_stat", "stat", "auth_stat", "f0", "f1", "f2", "payload_len", "cred_id",
              "cred_kind_len", "verf_id", "verf_kind_len"):
        assert np.array_equal(gm[f][ok], lm[f][ok]), f
    pay = ok & HM.has_payload(lm)
    i = np.nonzero(pay)[0]
    assert np.array_equal(gm["payload_off"][i].astype(np.int64) - i * head_len,
                          lm["payload_off"][i].astype(np.int64) - off[i].astype(np.int64))
    a, pa = L.resolve_unix(gm, gu, gs)
    b, pb = L.resolve_unix(lm, lu, np.where(ok, 0, 1))
    for k in ("stamp", "uid", "gid", "ngids", "name_len", "gids"):
        assert np.array_equal(pa.view(L.UNIX_DTYPE)[k][ok], pb.view(L.UNIX_DTYPE)[k][ok]), k


def _rng_bytes(n, seed):
    return np.random.default_rng(seed).bytes(n)


@pytest.mark.parametrize("policy", ["standard", "line"])
@pytest.mark.parametrize("mode", MODES)
def test_head_boundaries(R, codecs, oracle, mode, policy):
    codec = codecs[policy]
    big, S_ = HM.big_unix_call(21, payload=_rng_bytes(300, 1))
    assert S_ == 244
    short_verf = HM.call(22, HM.NONE, HM.auth(HM.AUTH_SHORT, _rng_bytes(200, 2)), _rng_bytes(700, 3))
    reply_far = HM.accepted(23, HM.auth(HM.AUTH_SHORT, _rng_bytes(200, 4)), 0, _rng_bytes(33, 5))
    name255, S255 = HM.big_unix_call(24, payload=_rng_bytes(100, 6), name_len=255)
    assert S255 == 384
    filler = HM.call(25, HM.NONE, HM.NONE, b"abc")
    recs = [filler, big, filler, short_verf, reply_far, filler, name255]
    BIG, VERF, REPLY, N255 = 1, 3, 4, 6
    short, ok = HM.HEAD_SHORT, (0, 0, 0)
    # the 255-byte name: 340 declared bytes, refused at the length word (byte 32) at every head_len
    for head_len, w_big, w_verf, w_reply in ((256, ok, ok, ok), (240, short, short, ok), (224, short, short, short),
                                             (160, short, short, short), (64, short, short, short),
                                             (384, ok, ok, ok), (368, ok, ok, ok)):
        exact = {BIG: w_big, VERF: w_verf, REPLY: w_reply, N255: (INVALID_LENGTH, 0, 0), 0: ok, 2: ok, 5: ok}
        got, want = _decode(R, codec, oracle, recs, head_len, mode, f"boundaries {head_len} {mode} {policy}", exact)
        assert not want[5][:6].any()                 # only the 255-byte name is an either-or record for the model
        gm, gu = got[0], got[1]
        if w_big == ok:
            u = gu[int(gm["cred_ref"][BIG])]
            assert int(u["name_off"]) == BIG * head_len + 44 and int(u["name_len"]) == 116 and int(u["ngids"]) == 16
            assert int(gm["payload_off"][BIG]) == BIG * head_len + 244 and int(gm["payload_len"][BIG]) == 300
        if w_verf == ok:
            assert int(gm["verf_ref"][VERF]) == VERF * head_len + 44 and int(gm["payload_len"][VERF]) == 700
        if w_reply == ok:
            assert int(gm["payload_off"][REPLY]) == REPLY * head_len + 228 and int(gm["payload_len"][REPLY]) == 33


@pytest.mark.parametrize("policy", ["standard", "line"])
def test_slot_ranks_shift_within_a_group(R, codecs, oracle, policy):
    recs = []
    for i in range(130):
        if i % 5 == 2:
            recs.append(HM.big_unix_call(i, payload=b"x" * 7)[0])              # header end 244: HEAD_SHORT at 160
        else:
            recs.append(HM.big_unix_call(i, payload=b"y" * (i % 9), name_len=i % 17, ngids=i % 5)[0])
    for mode in MODES:
        got, want = _decode(R, codecs[policy], oracle, recs, 160, mode, f"slot ranks {mode} {policy}")
        gs = got[2]
        assert (gs[2::5] == HM.DEC_BAD_EXTENT).all() and int((gs == 0).sum()) == 104
        ok = np.nonzero(gs == 0)[0]
        for g0 in (0, 64, 128):
            mine = ok[(ok >= g0) & (ok < g0 + 64)]
            assert got[0]["cred_ref"][mine].tolist() == list(range(2 * g0, 2 * g0 + len(mine)))


@pytest.fixture(scope="module")
def messages(oracle):
    """300 random messages as the oracle encodes them: (records, packed wire, offsets)."""
    wire, off, st, _ = oracle.encode_batch(L.build_batch(S.random_messages(300, seed=91, max_payload=1025)))
    assert not st.any()
    return [wire[int(off[i]):int(off[i + 1])] for i in range(300)], wire, off


@pytest.mark.parametrize("policy", ["standard", "line"])
@pytest.mark.parametrize("head_len", [64, 160, 736])
def test_results_do_not_depend_on_absent_bytes(R, codecs, oracle, messages, head_len, policy):
    recs = messages[0]
    assert sum(len(r) < head_len for r in recs) > 5 or head_len == 64
    for mode in MODES:
        a, _ = _decode(R, codecs[policy], oracle, recs, head_len, mode, f"fill 00 {head_len}", fill=0x00)
        b, want = _decode(R, codecs[policy], oracle, recs, head_len, mode, f"fill a5 {head_len}", fill=0xA5)
        for x, y in zip((a[0].view(np.uint8), a[2], a[3], a[4]), (b[0].view(np.uint8), b[2], b[3], b[4])):
            assert np.array_equal(x, y)
        if head_len == 736:
            assert not b[2].any()


@pytest.mark.parametrize("policy", ["standard", "line"])
@pytest.mark.parametrize("mode", MODES)
def test_constructed_mutants_give_their_exact_errors(R, codecs, oracle, mode, policy):
    plain = HM.call(31, HM.NONE, HM.NONE, _rng_bytes(1000, 7))
    unixc = HM.big_unix_call(32, payload=_rng_bytes(900, 8), name_len=9, ngids=3)[0]
    recs, exact = [plain, unixc], {}
    for src in (plain, unixc):
        for at, v, st in ((8, 7, (INVALID_MESSAGE_TYPE, 7, 0)), (12, 3, (INVALID_RPC_VERSION, 3, 0)),
                          (32, 201, (INVALID_LENGTH, 0, 0))):
            m = bytearray(src)
            m[at:at + 4] = HM.be(v)
            exact[len(recs)] = st
            recs.append(bytes(m))
    for head_len in (64, 160, 736):
        got, want = _decode(R, codecs[policy], oracle, recs, head_len, mode, f"mutants {head_len} {mode} {policy}", exact)
        assert want[5].tolist() == [False, False] + [True] * 6
        for i, st in exact.items():                  # ... which are the oracle's
            assert (int(want[2][i]), int(want[3][i]), int(want[4][i])) == st


# ---------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------
def _fragmented_slab(recs, seed, nseg=20):
    """Every record refragmented at a random max_frag in 1..64, the records
    dealt over nseg segments, most of which end in a pending run."""
    rng = np.random.default_rng(seed)
    sl = SM.Slab(front=int(rng.integers(0, 16)))
    cut = np.sort(rng.integers(0, len(recs) + 1, nseg - 1)).tolist()
    for lo, hi in zip([0] + cut, cut + [len(recs)]):
        data = b""
        for rec in recs[lo:hi]:
            mf = int(rng.integers(1, 65))
            data += FR.fragment(rec[4:], list(range(mf, len(rec) - 4, mf)))
        if rng.random() < 0.7:
            data += FS._pending(rng, int(rng.integers(1, 4)))
        sl.add(data, gap=int(rng.integers(0, 24)))
    return sl.done()


def test_end_to_end_frame_heads_decode(R, codecs, oracle, messages):
    recs = messages[0]
    slab, off, ln = _fragmented_slab(recs, 93)
    codec = codecs["standard"]
    start, flen, _, rows, fres = R.frame_host_fragment_streams(codec, slab, off, ln, with_seg=False)
    assert int(fres[2]) == 300 and int(fres[0]) > 3000 and (rows[:, 3] == 0).all()
    for head_len in (160, 736):
        m, g = _check_heads(R, codec, slab, start, flen, head_len, what=f"end to end {head_len}")
        assert int(g["result"][0]) == 300 and int(g["result"][3]) == 0
        assert g["rec_len"].tolist() == [len(r) for r in recs]
        for mode in MODES:
            for policy in ("standard", "line"):
                got = R.decode_host_heads(codecs[policy], g["heads"][:300 * head_len].tobytes(), head_len, g["rec_len"],
                                          mode)
                want = HM.decode_heads(oracle, recs, head_len, mode)
                assert not want[5].any()
                HM.check_decode(got, want, f"end to end {head_len} {mode} {policy}")
        gm, _, gs, _, _ = got
        assert (gs == 0).all() if head_len == 736 else 100 < int((gs == 0).sum()) < 300     # some headers reach past 160
        # every OK record's payload, gathered on the host through rec_frag / frag_pre
        checked = 0
        for i in np.nonzero((gs == 0) & HM.has_payload(gm))[0]:
            pos, plen = int(gm["payload_off"][i]) - int(i) * head_len, int(gm["payload_len"][i])
            assert pos + plen == len(recs[i])
            if plen:
                assert HM.gather(g, slab, start, flen, int(i), pos, plen) == recs[i][pos:], i
                assert slab[HM.locate(g, start, int(i), pos)] == recs[i][pos]
                checked += 1
        wm = want[0]
        assert checked == int(((want[2] == 0) & HM.has_payload(wm) & (wm["payload_len"] > 0)).sum()) > 40


def test_graph_capture_heads_then_decode(R, oracle, messages):
    """onc_codec_reserve, then onc_defragment_heads + onc_decode_heads captured
    on the codec's stream — every step is a kernel launch — and replayed on
    another slab copied into the same buffers. The captured calls run over
    `cap` extents: those past the framed ones are what the caller left there, a
    pending empty fragment kept at the buffer's end."""
    import torch
    recs = messages[0]
    slabs = []
    for seed in (96, 97):
        mine = recs[:150] if seed == 96 else recs[150:]
        slab, off, ln = _fragmented_slab(mine, seed, nseg=7)
        want = FS.frame_fragment_streams(slab, off, ln)
        slabs.append((slab, want.frag_start, want.frag_len, mine))
    size = max(len(x[0]) for x in slabs) + 16
    cap, head_len, n = 8192, 160, 150
    assert all(len(x[1]) < cap for x in slabs)
    s = torch.cuda.Stream()
    c = R.Codec(0, stream=s.cuda_stream, decode_policy=R.DECODE_POLICY_STANDARD)
    try:
        wire = torch.zeros(size + 32, dtype=torch.uint8, device="cuda")      # [size, size + 4): 00 00 00 00
        start = torch.full((cap + 1,), size, dtype=torch.int64, device="cuda")
        flen = torch.full((cap + 1,), 4, dtype=torch.int32, device="cuda")
        hbase, lo = R.aligned_bytes(cap * head_len, 0, "cuda")
        heads = hbase.data_ptr() + lo
        rec_len = torch.zeros(cap + 1, dtype=torch.int32, device="cuda")
        rec_frag = torch.zeros(cap + 2, dtype=torch.int64, device="cuda")
        frag_pre = torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
        status = torch.zeros(cap + 1, dtype=torch.int32, device="cuda")
        res = torch.zeros(6, dtype=torch.int64, device="cuda")
        d = R.DecodeBuffers(n)

        def work():
            c.defragment_heads(wire, start, flen, cap, head_len, heads, cap, rec_len, rec_frag, frag_pre, status, res)
            c.decode_heads(heads, head_len, rec_len, n, L.DECODE_SLICE, d.msgs, d.unix, d.status, d.aux0, d.aux1)

        def refresh(slab, fs, fl):
            wire[:len(slab)] = torch.from_numpy(np.frombuffer(slab, np.uint8).copy()).cuda()
            hbase.zero_()                            # (slot tails keep what an earlier run left)
            start.fill_(size)
            flen.fill_(4)
            start[:len(fs)] = torch.from_numpy(fs.view(np.int64).copy()).cuda()
            flen[:len(fl)] = torch.from_numpy(fl.view(np.int32).copy()).cuda()
            torch.cuda.synchronize()

        # without the reserve, the plan would grow its scratch inside the capture
        g0 = torch.cuda.CUDAGraph()
        err = None
        with torch.cuda.graph(g0, stream=s):
            try:
                c.defragment_heads(wire, start, flen, 1 << 20, head_len, heads, cap, rec_len, rec_frag, frag_pre, status,
                                   res)
            except R.CodecError as e:
                err = str(e)
        assert err is not None and "rc=-5" in err, err
        c.reserve(cap)
        refresh(*slabs[0][:3])
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            work()                                   # warm-up outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            work()
        torch.cuda.synchronize()
        slab, fs, fl, mine = slabs[1]
        refresh(slab, fs, fl)
        g.replay()
        torch.cuda.synchronize()
        nf = len(fs)
        m = HM.defragment_heads(slab, fs, fl, head_len)
        r6 = res.cpu().numpy().view(np.uint64)
        assert r6.tolist() == [n, nf, n * head_len, cap - nf, 0, int(m["result"][5])]
        assert np.array_equal(rec_len.cpu().numpy().view(np.uint32)[:n], m["rec_len"])
        assert np.array_equal(rec_frag.cpu().numpy().view(np.uint64)[:n + 1], m["rec_frag"])
        got_heads = hbase.cpu().numpy()[lo:lo + n * head_len]
        assert np.array_equal(got_heads, HM.expected_heads(m, head_len, n * head_len, 0))
        HM.check_decode(d.to_host(), HM.decode_heads(oracle, mine, head_len, L.DECODE_SLICE), "replayed heads + decode")
    finally:
        c.close()


# ---------------------------------------------------------------------------
# 4. the C++ mirror
# ---------------------------------------------------------------------------
def _fnv1a(b):
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


@pytest.mark.parametrize("retry", [False, True])
def test_cpp_mirror_fragmented_heads(oracle, messages, tmp_path, retry):
    """BatchDecoder::try_from_fragmented_heads against try_from_mixed_streams
    on the same slab (tests/cpp_heads/test_heads.cpp compares them record by
    record, payload bytes included), with and without a record whose header
    does not fit a 160-byte head, which forces the 736-byte retry."""
    exe = os.path.join(ROOT, "tests", "cpp_heads", "test_heads")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    recs = messages[0][:200]
    hdr_end = HM.decode_heads(oracle, recs, 160, L.DECODE_SLICE)
    recs = [r for r, st in zip(recs, hdr_end[2]) if st == 0][:90]           # headers that fit 160 bytes
    if retry:
        recs.insert(40, HM.big_unix_call(77, payload=b"retry me" * 20)[0])
    rng = np.random.default_rng(95)
    sl = SM.Slab(front=3)
    cut = np.sort(rng.integers(0, len(recs) + 1, 11)).tolist()
    for s, (lo, hi) in enumerate(zip([0] + cut, cut + [len(recs)])):
        data = b""
        for rec in recs[lo:hi]:
            mf = int(rng.integers(8, 200))
            data += rec if s % 3 == 0 else FR.fragment(rec[4:], list(range(mf, len(rec) - 4, mf)))
        if s % 4 == 1:
            data += FR._BE.pack(12) + b"pending run."
        sl.add(data, gap=int(rng.integers(0, 24)))
    slab, off, ln = sl.done()
    src, dst = str(tmp_path / "slab.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<QQ", len(off), len(slab)) + off.tobytes() + ln.tobytes() + slab)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0 and "PASS test_heads" in r.stdout, r.stdout + r.stderr
    out = open(dst, "rb").read()
    want = FS.frame_fragment_streams(slab, off, ln)
    n_rec, n_frags, n_multi, retried, head_len = struct.unpack_from("<QQQQQ", out)
    assert [n_rec, n_frags] == [len(recs), int(want.result[0])]
    assert n_multi == int(FS.defragment_extents(slab, want.frag_start, want.frag_len)["result"][5]) > 10
    assert (retried, head_len) == ((1, 736) if retry else (0, 160))
    rec_t = np.dtype([("st", "<i4"), ("xid", "<u4"), ("plen", "<u4"), ("fnv", "<u4"), ("pieces", "<u4")])
    got = np.frombuffer(out, rec_t, n_rec, 40)
    assert 40 + 20 * n_rec == len(out)
    wire = np.frombuffer(b"".join(recs) + b"\0" * 16, np.uint8).copy()
    o = np.concatenate(([0], np.cumsum([len(x) for x in recs]))).astype(np.uint64)
    om, _, ost, _, _ = oracle.decode_batch(wire, o, L.DECODE_SLICE)
    assert not ost.any() and not got["st"].any()
    assert np.array_equal(got["xid"], om["xid"]) and np.array_equal(got["plen"], om["payload_len"])
    w = wire.tobytes()
    assert got["fnv"].tolist() == [_fnv1a(w[int(a):int(a) + int(b)]) for a, b in zip(om["payload_off"], om["payload_len"])]
    assert int(got["pieces"].max()) > 3 and (got["pieces"][got["plen"] > 0] >= 1).all()
