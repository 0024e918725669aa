"""The host model of onc_defragment_heads and onc_decode_heads
(tests/heads_model.py) checked on the CPU: the gather model derived from the
packed reassembly against the header's serial loop written out on its own, the
payload locator against the packed records, and the decode model's rules on
records whose outcome can be stated by hand."""
import numpy as np
import pytest

import fragment_model as FR
import fragment_streams_model as FS
import heads_model as HM
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S

MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
INVALID_MESSAGE_TYPE, INVALID_LENGTH, INVALID_RPC_VERSION, INCOMPLETE_HEADER = 4, 10, 11, 2


def _stream(seed=5, nrec=40):
    rng = np.random.default_rng(seed)
    return b"".join(FS.record(rng, int(rng.integers(1, 7)), max_body=300) for _ in range(nrec)) + FS._pending(rng, 2)


@pytest.mark.parametrize("head_len", [64, 160, 736, 4096])
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_gather_model_is_the_serial_loop(head_len, order):
    wire, start, flen = FS.scatter(_stream(), order)
    full = HM.defragment_heads(wire, start, flen, head_len)
    n = len(full["status"])
    assert n == 40 and int(full["result"][3]) == 2 and int(full["result"][2]) == n * head_len
    for cap in (0, 1, n - 1, n, n + 3):
        a = HM.defragment_heads(wire, start, flen, head_len, cap)
        b = HM.serial_heads(wire, start, flen, head_len, cap)
        assert HM.same_heads(a, b) == [], (cap, HM.same_heads(a, b))
        assert a["status"].tolist() == [0 if r < cap else HM.ENC_WRITE_ZERO for r in range(n)]
    packed = FS.defragment_extents(wire, start, flen)
    assert np.array_equal(full["rec_len"], np.diff(packed["rec_off"].astype(np.int64)))
    assert full["result"][[0, 1, 3, 4, 5]].tolist() == packed["result"][[0, 1, 3, 4, 5]].tolist()
    for r, rec in enumerate(packed["records"]):
        assert full["slots"][r] == rec[:head_len]


def test_locator_finds_every_record_byte():
    wire, start, flen = FS.scatter(_stream(seed=6, nrec=12), "shuffled")
    m = HM.defragment_heads(wire, start, flen, 64)
    packed = FS.defragment_extents(wire, start, flen)
    for r, rec in enumerate(packed["records"]):
        for p in range(4, len(rec)):
            assert wire[HM.locate(m, start, r, p)] == rec[p], (r, p)
        assert HM.gather(m, wire, start, flen, r, 4, len(rec) - 4) == rec[4:]


def test_empty_and_pending_only():
    m = HM.serial_heads(b"", [], [], 64, 5)
    assert m["rec_frag"].tolist() == [0] and not m["result"].any()
    wire, start, flen = FS.scatter(FS.CONT0 + FR._BE.pack(3) + b"abc", "ascending")
    for f in (HM.serial_heads(wire, start, flen, 64, 5), HM.defragment_heads(wire, start, flen, 64, 5)):
        assert f["result"].tolist() == [0, 0, 0, 2, 3, 0] and f["rec_frag"].tolist() == [0]
        assert f["frag_pre"].tolist() == [0, 0]


def test_golden_error_vectors_are_shorter_than_the_default_head(golden):
    """So their outcome through onc_decode_heads is the oracle's, exactly, at
    every head_len >= 160. One vector is longer, unix_len_over_200 (240
    bytes): its error is the credential length word at byte 32 — a stated
    mutant position, below every head_len — checked before any later read
    (flavor.rs:83-85), so it is exact too and the GPU test states it."""
    n, longer = 0, []
    for sect in ("errors", "derived_errors"):
        for v in golden[sect]:
            rec = bytes.fromhex(v["hex"])
            if len(rec) >= 160:
                longer.append(v["name"])
                assert int.from_bytes(rec[32:36], "big") > 200 and rec[8:12] == HM.be(0) and rec[12:16] == HM.be(2)
                assert v["expect_by_mode"]["slice"]["status"] == v["expect_by_mode"]["bytes"]["status"] == INVALID_LENGTH
            n += 1
    assert n > 10 and longer == ["unix_len_over_200"]


@pytest.mark.parametrize("mode", MODES)
def test_decode_model_rules(oracle, mode):
    rng = np.random.default_rng(3)
    big, S_ = HM.big_unix_call(11, payload=rng.bytes(40))
    assert S_ == 244 and len(big) == 284
    short_verf = HM.call(12, HM.NONE, HM.auth(HM.AUTH_SHORT, rng.bytes(200)), rng.bytes(500))      # header end 244
    reply_far = HM.accepted(13, HM.auth(HM.AUTH_SHORT, rng.bytes(200)), 0, rng.bytes(9))            # stat word at 224, payload at 228
    plain = HM.call(14, HM.NONE, HM.NONE, rng.bytes(1000))                                          # header end 44
    mutants = [bytearray(plain) for _ in range(3)]
    mutants[0][8:12] = HM.be(7)                      # msg_type
    mutants[1][12:16] = HM.be(3)                     # rpc version
    mutants[2][32:36] = HM.be(201)                   # credential length
    recs = [big, short_verf, reply_far, plain, b"", b"\x80\x00"] + [bytes(x) for x in mutants]
    for head_len, want_short in ((256, []), (240, [0, 1]), (160, [0, 1, 2]), (64, [0, 1, 2])):
        msgs, unix, st, a0, a1, either = HM.decode_heads(oracle, recs, head_len, mode)
        for i in range(4):
            got = (int(st[i]), int(a0[i]), int(a1[i]))
            assert got == (HM.HEAD_SHORT if i in want_short else (0, 0, 0)), (head_len, i, got)
        if head_len == 240:
            assert reply_far[224:228] == HM.be(0) and int(st[2]) == 0       # the stat word ends at 228 <= 240
        assert st[4] == st[5] == INCOMPLETE_HEADER
        assert either.tolist() == [False] * 6 + [True] * 3
        assert (int(st[6]), int(a0[6])) == (INVALID_MESSAGE_TYPE, 7)
        assert (int(st[7]), int(a0[7])) == (INVALID_RPC_VERSION, 3)
        assert int(st[8]) == INVALID_LENGTH
        # an OK record: offsets relative to its slot, the true payload length
        assert int(msgs["payload_off"][3]) == 3 * head_len + 44 and int(msgs["payload_len"][3]) == 1000
        if 0 not in want_short:
            assert int(msgs["cred_ref"][0]) == 0 and int(unix["name_off"][0]) == 0 * head_len + 44
            assert int(unix["name_len"][0]) == 116 and int(unix["ngids"][0]) == 16
            assert int(msgs["payload_off"][0]) == 244 and int(msgs["payload_len"][0]) == 40


def test_decode_model_ranks_slots_per_64_records(oracle):
    """HEAD_SHORT records take no slot: the ranks of the AUTH_UNIX records
    after them in the same 64-record group move down."""
    recs = []
    for i in range(130):
        if i % 5 == 2:
            recs.append(HM.big_unix_call(i, payload=b"x" * 7)[0])              # header end 244: HEAD_SHORT at 160
        else:
            recs.append(HM.big_unix_call(i, payload=b"y" * (i % 9), name_len=i % 17, ngids=i % 5)[0])
    msgs, unix, st, a0, a1, either = HM.decode_heads(oracle, recs, 160, L.DECODE_SLICE)
    assert not either.any() and (st[2::5] == 106).all() and (np.delete(st, np.s_[2::5]) == 0).all()
    ok = np.nonzero(st == 0)[0]
    for g0 in (0, 64, 128):
        mine = ok[(ok >= g0) & (ok < g0 + 64)]
        assert msgs["cred_ref"][mine].tolist() == list(range(2 * g0, 2 * g0 + len(mine)))
    full = HM.decode_heads(oracle, recs, 256, L.DECODE_SLICE)
    assert not full[2].any() and full[0]["cred_ref"][:64].tolist() == list(range(64))
    i = int(ok[5])
    assert int(unix["name_off"][int(msgs["cred_ref"][i])]) == i * 160 + 44


def test_random_messages_model_equals_oracle_at_full_heads(oracle):
    """With 736-byte heads HEAD_SHORT cannot occur: the model is the oracle's
    decode, rebased."""
    wire, off, st, _ = oracle.encode_batch(L.build_batch(S.random_messages(200, seed=9, max_payload=900)))
    assert not st.any()
    recs = [wire[int(off[i]):int(off[i + 1])] for i in range(200)]
    for mode in MODES:
        om, ou, ost, _, _ = oracle.decode_batch(np.frombuffer(wire + b"\0" * 16, np.uint8).copy(), off, mode)
        msgs, unix, s2, _, _, either = HM.decode_heads(oracle, recs, HM.HEAD_FULL, mode)
        assert not s2.any() and not ost.any() and not either.any()
        pay = HM.has_payload(om)
        at = off[:-1].astype(np.int64)
        assert np.array_equal(msgs["payload_off"][pay].astype(np.int64) - np.arange(200)[pay] * HM.HEAD_FULL,
                              om["payload_off"][pay].astype(np.int64) - at[pay])
        assert np.array_equal(msgs["payload_len"], om["payload_len"])
        hdr = np.where(pay, om["payload_off"].astype(np.int64) - at, np.diff(at, append=int(off[-1])))
        assert int(hdr.max()) <= HM.HEAD_SPAN_MAX
