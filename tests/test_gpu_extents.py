"""onc_decode_extents on the GPU (decode.hip kExtents) against the CPU
oracle's decode of each record's own slice, in both modes and under both
pinned first-round policies: records in ascending, descending and permuted
address order, with gaps, repeated, a wave whose lowest window is its last
lane's (the minimum-base rule of the loaders, near and 2 GiB apart), bad
extents, and the per-connection flow end to end (onc_frame_streams first,
and the C++ mirror's try_from_streams on the same slab).

For the bad-extent cases the wire is a view inside a larger device tensor
whose surrounding bytes are valid records, and every bad extent but the
near-2^64 one (start past any wire: nothing is read for it) stays within 1 KiB
of the wire: a kernel that reads outside fails the comparison, not the run."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import frame_model as FM
import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
import streams_model as SM
from test_gpu_bounded import FRONT, PAD, Placed, check, expected
from test_gpu_parity import assert_decoded_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
POLICIES = ["standard", "line"]
U64_MAX = 2**64 - 1


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


def _dev(a, dtype):
    import torch
    a = np.append(np.ascontiguousarray(a, dtype), np.zeros(1, dtype))
    return torch.from_numpy(a.view({8: np.int64, 4: np.int32}[np.dtype(dtype).itemsize]).copy()).cuda()


def run_ext(R, codec, wire, wire_len, start, length, mode):
    n = len(start)
    b = R.DecodeBuffers(n)
    codec.decode_extents(wire, wire_len, _dev(start, np.uint64), _dev(length, np.uint32), n, mode, b.msgs, b.unix,
                         b.status, b.aux0, b.aux1)
    codec.sync()
    return b.to_host()


def reasons(start, length, wire_len):
    return [1 if int(s) > wire_len else 2 if int(l) > wire_len - int(s) else 0 for s, l in zip(start, length)]


def expect_extents(oracle, wire, start, length, wire_len, mode):
    """Output i = the oracle's decode of wire[start[i], start[i] + length[i])
    (106 / reason / 0 for an extent outside wire_len), AUTH_UNIX slots packed
    per 64 output records (test_gpu_bounded.expected)."""
    why = reasons(start, length, wire_len)
    lo = [int(s) for s in start]
    hi = [0 if y else int(s) + int(l) for s, l, y in zip(start, length, why)]
    return expected(oracle, wire, lo, hi, why, mode)


@pytest.fixture(scope="module")
def mixed(oracle):
    """200 mixed records back to back (FM.mixed_stream) at writer offset 3:
    (wire, start, length, device tensor)."""
    import torch
    buf = FM.mixed_stream(200, 53, 0, 300)
    starts, stop, st = FM.true_starts(buf)[:3]
    assert st == 0 and stop == len(buf) and len(starts) == 200
    w = np.concatenate([np.full(3, 0xEE, np.uint8), np.frombuffer(buf, np.uint8), np.zeros(16, np.uint8)])
    start = starts.astype(np.uint64) + np.uint64(3)
    length = np.diff(np.append(starts, stop)).astype(np.uint32)
    return w, start, length, torch.from_numpy(w).cuda()


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_contiguous_extents_equal_bounded_and_oracle(codecs, R, oracle, mixed, policy):
    w, start, length, dw = mixed
    off = np.append(start, start[-1] + np.uint64(length[-1]))
    T = int(off[-1])
    codec = codecs[policy]
    for mode in MODES:
        for n in (1, 63, 64, 65, 200):
            ora = oracle.decode_batch(w, off[:n + 1], mode)
            got = run_ext(R, codec, dw, T, start[:n], length[:n], mode)
            check(got, ora, f"extents n {n} mode {mode}")
            b = R.DecodeBuffers(n)
            codec.decode_bounded(dw, T, _dev(off[:n + 1], np.uint64), n, mode, b.msgs, b.unix, b.status, b.aux0,
                                 b.aux1)
            codec.sync()
            bd = b.to_host()
            assert_decoded_equal(got, bd, f"extents vs bounded n {n}")
            assert np.array_equal(got[0].view(np.uint8), bd[0].view(np.uint8))
        # trusted extents
        got = run_ext(R, codec, dw, U64_MAX, start, length, mode)
        check(got, oracle.decode_batch(w, off, mode), f"wire_len 2^64 - 1 mode {mode}")


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("order", ["reversed", "permuted", "thrice"])
def test_any_order(codecs, R, oracle, mixed, policy, order):
    """Output i is the decode of slice i wherever it lies; slots are grouped
    by output index. reversed: every wave's lowest window is its last lane's."""
    w, start, length, dw = mixed
    if order == "reversed":
        idx = np.arange(200)[::-1]
    elif order == "permuted":
        idx = np.random.default_rng(61).permutation(200)
    else:
        unix = int(np.nonzero(length > 120)[0][0])
        idx = np.concatenate([np.arange(70), [unix, unix, unix], np.arange(70, 130)])
    s, l = start[idx].copy(), length[idx].copy()
    for mode in MODES:
        want = expect_extents(oracle, w, s, l, len(w), mode)
        assert (want[2] == 0).sum() > 100
        check(run_ext(R, codecs[policy], dw, len(w), s, l, mode), want, f"{order} mode {mode}")
    if order == "thrice":
        m = want[0]
        assert np.array_equal(m[70:73]["xid"], np.repeat(m[70:71]["xid"], 3))


@pytest.mark.parametrize("policy", POLICIES)
def test_garbage_gaps(codecs, R, oracle, mixed, policy):
    import torch
    w, start, length, _ = mixed
    rng = np.random.default_rng(62)
    parts, s, pos = [], [], 0
    for i in range(130):
        gap = rng.integers(0, 40)
        parts.append(rng.integers(0, 256, gap, dtype=np.uint8))
        pos += int(gap)
        s.append(pos)
        parts.append(w[int(start[i]):int(start[i]) + int(length[i])])
        pos += int(length[i])
    g = np.concatenate(parts + [np.zeros(16, np.uint8)])
    s = np.array(s, np.uint64)
    dg = torch.from_numpy(g).cuda()
    for mode in MODES:
        want = expect_extents(oracle, g, s, length[:130], len(g), mode)
        check(run_ext(R, codecs[policy], dg, len(g), s, length[:130], mode), want, f"gaps mode {mode}")


@pytest.fixture(scope="module")
def unix16(oracle):
    """130 AUTH_UNIX Calls with 16 gids (headers that need a second round
    under the standard policy) mixed with short replies."""
    uw, uo, ust, _ = oracle.encode_batch(S.call_unix16(130, 40, seed=63))
    assert not ust.any()
    recs = [bytes(uw[int(uo[i]):int(uo[i + 1])]) for i in range(130)]
    for i in range(0, 130, 3):
        recs[i] = FM.reply28(i)
    w, o = L.records_from_wire(recs)
    o = np.asarray(o, np.uint64)
    w = np.concatenate([np.asarray(w, np.uint8)[:int(o[-1])], np.zeros(16, np.uint8)])
    return w, o[:-1].copy(), np.diff(o.astype(np.int64)).astype(np.uint32)


@pytest.mark.parametrize("policy", POLICIES)
def test_descending_windows_with_round2(codecs, R, oracle, unix16, policy):
    import torch
    w, start, length = unix16
    assert int(length.max()) >= 140
    s, l = start[::-1].copy(), length[::-1].copy()
    dw = torch.from_numpy(w).cuda()
    for mode in MODES:
        want = expect_extents(oracle, w, s, l, len(w), mode)
        assert (want[2] == 0).all()
        check(run_ext(R, codecs[policy], dw, len(w), s, l, mode), want, f"descending round 2 mode {mode}")


@pytest.mark.parametrize("policy", POLICIES)
def test_far_windows_low_record_last(codecs, R, oracle, unix16, policy):
    """Lanes 0..62 of the first wave lie 2 GiB above its last lane's record:
    with the resource based at the wave's lowest window they are out of its
    reach, so the wave takes the per-lane loads (a base taken from the first
    lane would give that last lane a negative offset). The following waves
    are near and cooperative."""
    import torch
    w, start, length = unix16
    far = 1 << 31
    n = len(start)
    dw = torch.zeros(far + len(w) + 16, dtype=torch.uint8, device="cuda")
    dw[:len(w)] = torch.from_numpy(w).cuda()
    dw[far:far + len(w)] = torch.from_numpy(w).cuda()
    host = np.zeros(far + len(w) + 16, np.uint8)                # zero pages in between: never touched
    host[:len(w)] = w
    host[far:far + len(w)] = w
    s = start + np.uint64(far)
    s[63] = start[1]                                            # an AUTH_UNIX call, low, last in its wave
    l = length.copy()
    l[63] = length[1]
    try:
        for mode in MODES:
            want = expect_extents(oracle, host, s, l, len(host), mode)
            assert (want[2] == 0).all() and int(want[0]["payload_off"][63]) < far <= int(want[0]["payload_off"][62])
            check(run_ext(R, codecs[policy], dw, len(host), s, l, mode), want, f"far windows mode {mode}")
    finally:
        del dw
        torch.cuda.empty_cache()
    assert n == 130


@pytest.mark.parametrize("policy", POLICIES)
def test_bad_extents_leave_neighbours_alone(codecs, R, oracle, mixed, policy):
    w, start, length, _ = mixed
    fw, fo, fst, _ = oracle.encode_batch(S.mixed(700, seed=77, pmin=0, pmax=200, exotic=0.2))
    filler = np.frombuffer(fw, np.uint8)
    assert not fst.any() and filler.size >= PAD + 16
    body = w[3:3 + int(start[-1]) - 3 + int(length[-1])]        # the records alone
    T = len(body)
    pl = Placed(filler, body)
    s = start - np.uint64(3)
    l = length.copy()
    s[10] = T + 1                                               # starts past the wire
    s[20] = T + 700
    l[70] = T - int(s[70]) + 1                                  # ends past it by one byte
    s[64], l[64] = np.uint64(2**64 - 8), 16                     # start + length wraps: never summed
    s[130], l[130] = T, 0                                       # the legal empty record at wire_len
    s[131], l[131] = T, 1
    why = reasons(s, l, T)
    assert {i: y for i, y in enumerate(why) if y} == {10: 1, 20: 1, 64: 1, 70: 2, 131: 2}
    both = np.concatenate([body, filler[:PAD]])
    for mode in MODES:
        want = expect_extents(oracle, both, s, l, T, mode)
        assert want[2][130] == 2 and (want[2] == 0).sum() > 150
        g = run_ext(R, codecs[policy], pl, T, s, l, mode)
        check(g, want, f"bad extents mode {mode}")
        for i, y in enumerate(why):
            if y:
                assert (g[2][i], g[3][i], g[4][i]) == (106, y, 0), i
    assert FRONT > 0


# ---------------------------------------------------------------------------
# end to end: a slab of connection buffers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_connection_slab_end_to_end(codecs, R, oracle, policy):
    slab, off, ln = SM.connection_slab()
    host = np.frombuffer(slab, np.uint8)
    want = SM.frame_streams(slab, off, ln)
    codec = codecs[policy]
    start, length, seg, rows, res = R.frame_host_streams(codec, slab, off, ln)
    assert np.array_equal(res, want.result) and np.array_equal(rows, want.rows)
    assert np.array_equal(start, want.rec_start) and np.array_equal(length, want.rec_len)
    assert np.array_equal(seg, want.rec_seg)
    for mode in MODES:
        got = R.decode_host_extents(codec, host, start, length, mode)
        exp = expect_extents(oracle, host, start, length, len(host), mode)
        assert (exp[2] == 0).sum() > 500
        check(got, exp, f"slab mode {mode}")
        # per connection: the oracle's own framing + decode of that buffer
        for c in (0, 1, 37, 61, 99):
            buf = slab[int(off[c]):int(off[c]) + int(ln[c])]
            o, n, consumed, st, a0, a1 = oracle.frame_stream(buf)
            assert tuple(int(x) for x in rows[c][1:]) == (n, consumed, st, a0, a1)
            om = oracle.decode_batch(np.frombuffer(buf + b"\0" * 16, np.uint8), o, mode)
            k = int(rows[c][0])
            assert np.array_equal(got[2][k:k + n], om[2]) and np.array_equal(got[0]["xid"][k:k + n], om[0]["xid"])


def test_cpp_mirror_streams(oracle):
    """BatchDecoder::try_from_streams (tests/cpp_streams/test_streams.cpp) on
    the same slab, staged and through a HostRegistration."""
    exe = os.path.join(ROOT, "tests", "cpp_streams", "test_streams")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    slab, off, ln = SM.connection_slab()
    body = slab[:100 * SM.SLOT]
    want = SM.frame_streams(body, off, ln)
    host = np.frombuffer(body + b"\0" * 16, np.uint8)
    exp = expect_extents(oracle, host, want.rec_start, want.rec_len, len(body), L.DECODE_SLICE)
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "slab.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<QQ", len(off), len(body)) + off.tobytes() + ln.tobytes() + body)
        r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        print(r.stdout)
        print(r.stderr)
        assert r.returncode == 0 and "PASS test_streams" in r.stdout, r.stdout + r.stderr
        out = open(dst, "rb").read()
    n = struct.unpack_from("<Q", out)[0]
    assert n == int(want.result[0])
    rows = np.frombuffer(out, np.uint64, 600, 8).reshape(100, 6)
    assert np.array_equal(rows, want.rows)
    recs = np.frombuffer(out, np.dtype([("st", "<i4"), ("xid", "<u4"), ("poff", "<u8"), ("plen", "<u4")]), n, 8 + 4800)
    assert np.array_equal(recs["st"], exp[2])
    ok = exp[2] == 0
    assert np.array_equal(recs["xid"][ok], exp[0]["xid"][ok])
    call = ok & (exp[0]["msg_type"] == L.MSG_CALL)
    assert call.sum() > 100
    assert np.array_equal(recs["poff"][call], exp[0]["payload_off"][call])
    assert np.array_equal(recs["plen"][call], exp[0]["payload_len"][call])
