"""The host model of the framer (tests/frame_model.py) against the CPU
oracle, and the preconditions of every stream the framer edge tests
(tests/test_gpu_frame_edges.py) build: each stream provably reaches the case
it is named for — starts per chunk around kStartsCap, marks across chunk
boundaries, off-chain guesses inside nested payloads, false stops, failures
spread over the three levels of the flag hierarchy. CPU only."""
import numpy as np
import pytest

import frame_model as M
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S


def _same_as_oracle(oracle, buf, max_records=None):
    ts, stop, st, a0, a1 = M.true_starts(buf, max_records)
    o = oracle.frame_stream(buf, max_records)
    assert (len(ts), stop, st, a0, a1) == o[1:], ((len(ts), stop, st, a0, a1), o[1:])
    assert np.array_equal(np.append(ts, stop).astype(np.uint64), o[0])


def _parity_valid_streams(oracle):
    """The streams of test_gpu_parity.test_frame_stream_valid_streams."""
    for hb in (S.call_none(5000, 256), S.mixed(3000, seed=3, pmin=0, pmax=5000, exotic=0.2),
               L.build_batch(S.random_messages(3000, seed=8, max_payload=300))):
        wire = oracle.encode_batch(hb)[0]
        yield wire, None
        for cut in (len(wire) - 1, len(wire) - 3, len(wire) // 2, 5, 2, 0):
            yield wire[:cut], None
        for m in (1, 7, hb.n // 2, hb.n - 1, hb.n, hb.n + 5):
            yield wire, m


def _parity_adversarial_streams(oracle):
    """The streams of test_gpu_parity.test_frame_stream_adversarial."""
    rng = np.random.default_rng(4)
    inner = oracle.encode_batch(S.mixed(400, seed=9, pmin=0, pmax=900))[0]
    msgs = []
    for i in range(600):
        k = int(rng.integers(0, len(inner) - 2000))
        msgs.append({"xid": i, "type": "call", "program": 1, "program_version": 1, "procedure": 1,
                     "cred": {"kind": "none", "data": None}, "verf": {"kind": "none", "data": None},
                     "payload": inner[k:k + int(rng.integers(0, 2000))].hex()})
    yield oracle.encode_batch(L.build_batch(msgs))[0]
    parts = []
    for i in range(3000):
        kind = int(rng.integers(0, 3))
        body = rng.bytes(int(rng.integers(0, 17)) if kind < 2 else int(rng.integers(3000, 9000)))
        parts.append(((len(body)) | 0x80000000).to_bytes(4, "big") + body)
    stream = b"".join(parts)
    yield stream
    bad = bytearray(stream)
    j = len(b"".join(parts[:1500]))
    bad[j] &= 0x7F
    yield bytes(bad)
    yield stream[:j] + rng.bytes(50000)
    yield rng.bytes(100000)


def test_true_starts_is_the_oracle_loop_on_the_parity_streams(oracle):
    for buf, m in _parity_valid_streams(oracle):
        _same_as_oracle(oracle, buf, m)
    for buf in _parity_adversarial_streams(oracle):
        _same_as_oracle(oracle, buf)


def test_model_guess_rules():
    """The guess rules on hand-made bytes: chunk 0 guesses 0; a plausible
    start whose successor is implausible is no guess; one whose successor
    lies within 16 bytes of the end is; positions in the last 15 bytes are
    no candidates."""
    a, b = M.reply28(1), M.call(2)
    # 0: opaque(64)  64: a  92: b  136: a  164: opaque(24)  188: a  216: end
    buf = M.opaque(b"\x01" * 60) + a + b + a + M.opaque(b"\x02" * 20) + a
    assert [M.plausible(buf, p) for p in (64, 92, 136, 164, 188)] == [True, True, True, False, True]
    assert list(M.guesses(buf, 64)) == [0, 64, 188, -1]       # 136's successor (164) is implausible
    f = M.chunk_flags(buf, 64)
    assert list(f["on_chain"]) == [True, True, True, False] and list(f["starts"]) == [1, 2, 3, 0]
    assert list(f["exit"]) == [1, 2, -1, -1] and list(f["stop_st"]) == [-1, -1, M.OK, -1]
    assert list(f["fail"]) == [False, True, False, False]     # chunk 1's chain lands on 136, chunk 2 guessed 188
    assert len(M.candidates(a[:15])) == 0 and list(M.candidates(a + a[:15])) == [0]


# ---------------------------------------------------------------------------
# (a) starts per chunk around kStartsCap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk,want", [(1764, {63}), (1792, {64}), (1820, {65}), (1800, {64, 65})])
def test_replies_starts_per_chunk(oracle, chunk, want):
    buf = M.replies_stream()
    _same_as_oracle(oracle, buf)
    f = M.chunk_flags(buf, chunk)
    assert set(f["starts"][:-1].tolist()) == want, M.starts_histogram(buf, chunk)
    assert f["on_chain"].all() and (f["g"] >= 0).all() and not f["fail"].any()


@pytest.mark.parametrize("first_len", [4, 8, 12])
def test_opaque16_no_guess_and_starts_around_cap(oracle, first_len):
    buf = M.opaque16_stream(first_len)
    _same_as_oracle(oracle, buf)
    f = M.chunk_flags(buf, 1024)
    assert (f["g"][1:] == -1).all(), "no chunk but chunk 0 has a guess: the walk re-chases every chunk"
    assert f["fail"][0]
    assert {63, 64, 65} <= set(f["starts"].tolist()), M.starts_histogram(buf, 1024)


# ---------------------------------------------------------------------------
# (b), (d): the mixed streams
# ---------------------------------------------------------------------------
def test_mixed_streams(oracle):
    buf = M.edge_stream()
    _same_as_oracle(oracle, buf)
    assert len(M.true_starts(buf)[0]) == 2000
    cut = M.cut_stream()
    _same_as_oracle(oracle, cut)
    assert len(M.true_starts(cut)[0]) == 200 and 12_000 <= len(cut) <= 20_000
    for n in list(range(0, 40)) + [len(cut) - k for k in range(0, 41)]:
        _same_as_oracle(oracle, cut[:n])
    for m in (0, 1, 199, 200, 201, 202):
        _same_as_oracle(oracle, cut, m)


# ---------------------------------------------------------------------------
# (c) marks straddling chunk boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plausible", "opaque"])
@pytest.mark.parametrize("chunk", [64, 100])
def test_straddle_every_offset(oracle, chunk, kind):
    buf = M.straddle_stream(chunk, kind)
    _same_as_oracle(oracle, buf)
    assert M.true_starts(buf)[1:3] == (len(buf), M.OK)
    assert M.straddle_offsets(buf, chunk) == set(M.STRADDLE_D)


# ---------------------------------------------------------------------------
# (e) nested streams and stale flags
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("chunk,inner,variant,placement,gap", M.NESTED_CASES)
def test_nested_preconditions(oracle, chunk, inner, variant, placement, gap):
    buf, info = M.nested_stream(chunk, inner, variant, placement, gap)
    _same_as_oracle(oracle, buf)
    # the inner stream ends exactly `gap` bytes before the payload's (= the outer record's) end
    assert info["gap"] == gap and (gap == 0) == (variant == 1)
    if gap:
        assert info["gap_pos"] == info["end"] - gap
        assert not any(b & 0x80 for b in buf[info["gap_pos"]:info["end"]]), "gap bytes have the high bit clear"
        inner_ts = M.true_starts(buf[info["outer"] + 44:info["gap_pos"]])
        assert inner_ts[1:3] == (info["gap_pos"] - info["outer"] - 44, M.OK), "a valid stream up to the gap"
    s = M.check_nested(buf, chunk, info, placement)
    print(f"nested chunk {chunk} variant {variant} {placement} gap {gap}: {s}")


# ---------------------------------------------------------------------------
# (f) flag hierarchy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.HIER_LAYOUTS))
def test_hierarchy_preconditions(oracle, name):
    buf, info = M.hier_stream(name)
    _same_as_oracle(oracle, buf)
    s = M.check_hier(buf, info, name)
    print(f"hierarchy {name}: {s}")


# ---------------------------------------------------------------------------
# (g), (h)
# ---------------------------------------------------------------------------
def test_tiny_and_large_streams(oracle):
    for buf in M.tiny_buffers():
        _same_as_oracle(oracle, buf)
    ts, stop, st, a0, a1 = M.true_starts(b"\xff\xff\xff\xff" + b"\x00" * 40)
    assert (st, a0, a1) == (M.INCOMPLETE_MESSAGE, 44, ((1 << 31) + 3) & 0xFFFFFFFF)
    z = M.zero_records()
    _same_as_oracle(oracle, z)
    assert M.starts_histogram(z, 64) == {16: 250} and M.starts_histogram(z, 1024) == {160: 1, 256: 15}
    for nbytes in (100, 12 << 20, 17 << 20):
        buf = M.big_filler_stream(nbytes)
        _same_as_oracle(oracle, buf)
        assert M.true_starts(buf)[1:3] == (len(buf), M.OK)
    # (h): the last stream needs more chunks of 64 bytes than the scratch the
    # hierarchy stream left (sizes double from 4096 chunks), so it grows
    cap = 4096
    while cap < (M.HIER_BYTES + 63) // 64:
        cap *= 2
    assert (len(M.big_filler_stream(12 << 20)) + 63) // 64 <= cap < (len(M.big_filler_stream(17 << 20)) + 63) // 64
