"""Bounded decode on the GPU (onc_decode_bounded, onc_decode_lengths_bounded,
onc_decode_body_bounded; decode.hip kBound) against the CPU oracle.

Every wire is a view inside a larger device tensor with at least 64 KiB of
valid records on either side, and every bad offset or length stays within
about 1 KiB of the wire: a decoder without the bound reads valid records and
answers OK (or some reference error) where 106 is due, so a wrong build fails
these tests by comparison and never by faulting. Expected values: the oracle
on each good record's own slice, ONC_DEC_BAD_EXTENT / reason / 0 with a zeroed
descriptor for the bad ones, and the AUTH_UNIX slots packed per 64-record
group over the OK records (`expected`, itself checked against the oracle's
batch decode on good input). Both modes, both first-round policies."""
import os
import struct
import subprocess

import numpy as np
import pytest

import onc_rpc_amd.layout as L
import onc_rpc_amd.synth as S
from test_gpu_parity import all_golden_records, assert_decoded_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [L.DECODE_SLICE, L.DECODE_BYTES]
PAD = 1 << 16                     # valid records on either side of the wire
FRONT = PAD + 5                   # the wire starts at byte 5 of a 16-byte granule
POLICIES = ["standard", "line"]


@pytest.fixture(scope="module")
def R():
    import onc_rpc_amd.runtime as R
    return R


@pytest.fixture(scope="module")
def codecs(R):
    """(policy, force_scan) -> codec: the first-round policy pinned, the
    lengths form's scanned-block path forced or not."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pol = {"standard": R.DECODE_POLICY_STANDARD, "line": R.DECODE_POLICY_LINE}
    cs = {(p, fs): R.Codec(0, decode_policy=pol[p], force_scan=fs) for p in POLICIES for fs in (False, True)}
    yield cs
    for c in cs.values():
        c.close()


def _split(wire, off):
    return [bytes(wire[int(off[i]):int(off[i + 1])]) for i in range(len(off) - 1)]


@pytest.fixture(scope="module")
def filler(oracle):
    """>= PAD + 16 bytes of back-to-back valid records."""
    wire, off, st, _ = oracle.encode_batch(S.mixed(700, seed=77, pmin=0, pmax=200, exotic=0.2))
    assert (st == 0).all()
    a = np.frombuffer(wire, np.uint8)
    assert a.size >= PAD + 16
    return a


class Placed:
    """`wire` inside a larger buffer: FRONT bytes of records before it, PAD
    after it. data_ptr() is the wire's first byte; dev = a device tensor, or
    a HostMapped buffer (the kernels read host memory in place)."""

    def __init__(self, filler, wire, mapped_codec=None, R=None):
        import torch
        big = np.concatenate([filler[-FRONT:], np.asarray(wire, np.uint8), filler[:PAD]])
        if mapped_codec is None:
            self.buf = torch.from_numpy(big).cuda()
        else:
            self.buf = R.HostMapped.from_array(mapped_codec, big)
        self.n = len(wire)

    def data_ptr(self):
        return self.buf.data_ptr() + FRONT


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).view({8: np.int64, 4: np.int32}[np.dtype(dtype).itemsize])
                            .copy()).cuda()


def run_off(R, codec, wire, wire_len, off, mode, bounded=True):
    n = len(off) - 1
    o = _dev(off, np.uint64)
    b = R.DecodeBuffers(n)
    if bounded:
        codec.decode_bounded(wire, wire_len, o, n, mode, b.msgs, b.unix, b.status, b.aux0, b.aux1)
    else:
        codec.decode(wire, o, n, mode, b.msgs, b.unix, b.status, b.aux0, b.aux1)
    codec.sync()
    return b.to_host()


def run_len(R, codec, wire, wire_len, lens, base, mode, bounded=True):
    import torch
    n = len(lens)
    rl = _dev(lens, np.uint32)
    ro = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    b = R.DecodeBuffers(n)
    if bounded:
        codec.decode_lengths_bounded(wire, wire_len, rl, n, base, mode, b.msgs, b.unix, b.status, b.aux0, b.aux1,
                                     rec_off=ro)
    else:
        codec.decode_lengths(wire, rl, n, base, mode, b.msgs, b.unix, b.status, b.aux0, b.aux1, rec_off=ro)
    codec.sync()
    return b.to_host(), ro.cpu().numpy().view(np.uint64).copy()


def run_body(R, codec, root, wire, wire_len, off, mode, param, bounded=True):
    import torch
    n = len(off) - 1
    o = _dev(off, np.uint64)
    prm = _dev(param, np.uint32)
    b = R.DecodeBuffers(n)
    cons = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    if bounded:
        codec.decode_body_bounded(root, wire, wire_len, o, n, mode, b.msgs, b.unix, b.status, b.aux0, b.aux1,
                                  param=prm, consumed=cons)
    else:
        codec.decode_body(root, wire, o, n, mode, b.msgs, b.unix, b.status, b.aux0, b.aux1, param=prm, consumed=cons)
    codec.sync()
    return b.to_host(), cons.cpu().numpy().view(np.uint32).copy()


def reasons_off(off, wire_len):
    """The issue's order: 3 = offsets decrease, 1 = start past, 2 = end past."""
    lo = [int(x) for x in off[:-1]]
    hi = [int(x) for x in off[1:]]
    return [3 if h < l else 1 if l > wire_len else 2 if h > wire_len else 0 for l, h in zip(lo, hi)]


def expected(oracle, wire, lo, hi, reason, mode, root=None, param=None):
    """(msgs, unix, status, aux0, aux1, consumed): the oracle on every good
    record's own slice wire[lo[i]:hi[i]] (a bad one presented as an empty
    slice takes no part), 106 / reason / 0 for the bad ones, and the layout of
    include/onc_rpc.h onc_decoded: a 64-record group's OK records put their
    AUTH_UNIX sets in consecutive slots from 128 g (the oracle's batch decode
    does the same: test_parity_on_good_input checks this against it)."""
    lib = oracle.load()
    n = len(lo)
    w = np.ascontiguousarray(wire, np.uint8)
    msgs, unix = np.zeros(n, L.MSG_DTYPE), np.zeros(2 * n, L.UNIX_DTYPE)
    st, a0, a1 = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    cons = np.zeros(n, np.uint32)
    k = 0
    for i in range(n):
        if i % 64 == 0:
            k = 0
        if reason[i]:
            st[i], a0[i] = L.DEC_BAD_EXTENT, reason[i]
            continue
        a, b = int(lo[i]), int(hi[i])
        assert 0 <= a <= b <= w.size
        u = np.zeros(2, L.UNIX_DTYPE)
        m, x0, x1, c = msgs[i:i + 1], a0[i:i + 1], a1[i:i + 1], cons[i:i + 1]
        if root is None:
            st[i] = lib.oracle_decode_message(w.ctypes.data, w.ctypes.data + a, b - a, mode, 2 * i, m.ctypes.data,
                                              u.ctypes.data, x0.ctypes.data, x1.ctypes.data)
        else:
            st[i] = lib.oracle_decode_body(root, w.ctypes.data, w.ctypes.data + a, b - a, mode,
                                           int(param[i]) if param is not None else 0, 2 * i, m.ctypes.data,
                                           u.ctypes.data, x0.ctypes.data, x1.ctypes.data, c.ctypes.data)
        if st[i] != 0:
            continue
        call = int(m["msg_type"][0]) == L.MSG_CALL
        cred = call and (int(m["cred_kind_len"][0]) >> 24) == L.KIND_UNIX
        verf = (call or int(m["reply_stat"][0]) == L.REPLY_ACCEPTED) and \
            (int(m["verf_kind_len"][0]) >> 24) == L.KIND_UNIX and \
            root not in (L.ROOT_AUTH_FLAVOR, L.ROOT_AUTH_UNIX_PARAMS)
        g = 2 * (i - i % 64)
        if cred:
            msgs["cred_ref"][i] = g + k
            unix[g + k] = u[0]
            k += 1
        if verf:
            msgs["verf_ref"][i] = g + k
            unix[g + k] = u[1]
            k += 1
    return msgs, unix, st, a0, a1, cons


def check(got, want, what):
    """Bit-exact: statuses, aux, descriptors (zeroed for every failed record),
    the AUTH_UNIX slots the OK records name."""
    assert_decoded_equal(got[:5], want[:5], what)
    bad = np.nonzero(want[2] != 0)[0]
    assert not got[0].view(np.uint8).reshape(-1, 64)[bad].any(), f"{what}: a failed record's descriptor is not zero"


@pytest.fixture(scope="module")
def good(oracle, golden, filler):
    """The golden records (error vectors included) + S.mixed(300, exotic=0.3)
    at writer offset 5, with the oracle's decode per mode."""
    recs, _ = all_golden_records(golden)
    wire, off, st, _ = oracle.encode_batch(S.mixed(300, exotic=0.3))
    assert (st == 0).all()
    recs = recs + _split(wire, off)
    w, o = L.records_from_wire(recs)
    o = np.asarray(o, np.uint64)
    w = np.asarray(w, np.uint8)[:int(o[-1])]
    return {"wire": w, "off": o, "placed": Placed(filler, w),
            "oracle": {m: oracle.decode_batch(w, o, m) for m in MODES}}


# ---------------------------------------------------------------------------
# 1. parity on good input
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_parity_on_good_input(codecs, R, oracle, good, policy):
    w, off, pl = good["wire"], good["off"], good["placed"]
    n, T = len(off) - 1, len(w)
    lens = np.diff(off.astype(np.int64)).astype(np.uint32)
    for mode in MODES:
        ora = good["oracle"][mode]
        # this file's expected-value builder is the oracle's batch decode
        exp = expected(oracle, w, off[:-1], off[1:], [0] * n, mode)
        assert_decoded_equal(exp[:5], ora, "expected() vs oracle")
        assert np.array_equal(exp[1].view(np.uint8), ora[1].view(np.uint8))
        codec = codecs[policy, False]
        gb = run_off(R, codec, pl, T, off, mode)
        gu = run_off(R, codec, pl, T, off, mode, bounded=False)
        check(gb, ora, f"bounded offsets mode {mode}")
        assert_decoded_equal(gb, gu, f"bounded vs unbounded offsets mode {mode}")
        for k in range(3):                             # status, aux0, aux1: bit-equal
            assert np.array_equal(gb[2 + k], gu[2 + k])
        for fs in (False, True):
            for m in (1, 64, 65, 300):                 # one workgroup; fused / scanned blocks
                codec = codecs[policy, fs]
                sub = tuple(x[:2 * m] if j == 1 else x[:m] for j, x in enumerate(ora))
                Tm = int(off[m])
                lb, rb = run_len(R, codec, pl, Tm, lens[:m], 0, mode)
                lu, ru = run_len(R, codec, pl, Tm, lens[:m], 0, mode, bounded=False)
                what = f"lengths n {m} scan {fs} mode {mode}"
                check(lb, sub, "bounded " + what)
                assert_decoded_equal(lb, lu, "bounded vs unbounded " + what)
                assert np.array_equal(rb, off[:m + 1]) and np.array_equal(ru, rb), what
        # the whole batch through the lengths form too
        lb, rb = run_len(R, codecs[policy, False], pl, T, lens, 0, mode)
        check(lb, ora, f"bounded lengths all mode {mode}")
        assert np.array_equal(rb, off)


# ---------------------------------------------------------------------------
# 2. exact fit and one short
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_exact_fit_and_one_short(codecs, R, oracle, good, policy):
    w, off, pl = good["wire"], good["off"], good["placed"]
    n, T = len(off) - 1, int(good["off"][-1])
    lens = np.diff(off.astype(np.int64)).astype(np.uint32)
    codec = codecs[policy, False]
    assert lens[-1] > 0
    for mode in MODES:
        ora = good["oracle"][mode]
        # wire_len = the end of the last record: all as before
        check(run_off(R, codec, pl, T, off, mode), ora, "exact fit, offsets")
        check(run_len(R, codec, pl, T, lens, 0, mode)[0], ora, "exact fit, lengths")
        # one byte short: only the last record, which ends past the wire
        short = expected(oracle, w, off[:-1], off[1:], [0] * (n - 1) + [2], mode)
        g = run_off(R, codec, pl, T - 1, off, mode)
        check(g, short, "one short, offsets")
        assert g[2][-1] == 106 and g[3][-1] == 2 and g[4][-1] == 0
        assert np.array_equal(g[2][:-1], ora[2][:-1])
        lg, ro = run_len(R, codec, pl, T - 1, lens, 0, mode)
        check(lg, short, "one short, lengths")
        assert np.array_equal(ro, off)
        # an empty record appended at b == wire_len: a legal empty slice
        off2 = np.concatenate([off, off[-1:]])
        want = expected(oracle, w, off2[:-1], off2[1:], [0] * (n + 1), mode)
        assert want[2][-1] == 2                        # IncompleteHeader: what an empty record decodes to
        check(run_off(R, codec, pl, T, off2, mode), want, "empty record at the end, offsets")
        check(run_len(R, codec, pl, T, np.append(lens, np.uint32(0)), 0, mode)[0], want,
              "empty record at the end, lengths")


# ---------------------------------------------------------------------------
# 3. offset form, adversarial
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def adversarial(oracle, filler):
    """200 records (four waves); record 150 an AUTH_UNIX Call with 16 gids
    (its header needs a second round under the standard policy)."""
    wire, off, st, _ = oracle.encode_batch(S.mixed(200, seed=91, pmin=0, pmax=200, exotic=0.3))
    assert (st == 0).all()
    recs = _split(wire, off)
    uw, uo, ust, _ = oracle.encode_batch(S.call_unix16(1, 40, seed=92))
    assert ust[0] == 0 and len(uw) >= 140
    recs[150] = bytes(uw)
    w, o = L.records_from_wire(recs)
    o = np.asarray(o, np.uint64)
    w = np.asarray(w, np.uint8)[:int(o[-1])]
    T = int(o[-1])
    r = o.copy()
    r[20] = o[21] + np.uint64(8)        # 19 runs into 21 (good extent); 20: offsets decrease, mid-wave
    r[100] = T + 64                     # 99 ends past the wire
    r[101] = T + 128                    # 100 starts past it; 101: offsets decrease
    r[128] = o[129] + np.uint64(4)      # 128: offsets decrease, lane 0 of the third wave
    r[151] = T + 200                    # 150, the AUTH_UNIX call, ends past the wire; 151: offsets decrease
    r[200] = T + 1000                   # 199 ends past the wire
    return {"wire": w, "off": r, "T": T, "placed": Placed(filler, w)}


@pytest.mark.parametrize("policy", POLICIES)
def test_offsets_adversarial(codecs, R, oracle, adversarial, filler, policy):
    w, r, T, pl = (adversarial[k] for k in ("wire", "off", "T", "placed"))
    why = reasons_off(r, T)
    assert {i: why[i] for i in range(200) if why[i]} == {20: 3, 99: 2, 100: 1, 101: 3, 128: 3, 150: 2, 151: 3, 199: 2}
    # good slices may run into the records after them, never past T
    both = np.concatenate([w, filler[:PAD]])
    for mode in MODES:
        want = expected(oracle, both, r[:-1], r[1:], why, mode)
        assert (want[2] == 0).sum() > 150
        g = run_off(R, codecs[policy, False], pl, T, r, mode)
        check(g, want, f"adversarial offsets mode {mode}")
        for i, y in enumerate(why):
            if y:
                assert (g[2][i], g[3][i], g[4][i]) == (106, y, 0), i


# ---------------------------------------------------------------------------
# 4. lengths form, adversarial
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("force_scan", [False, True])
def test_lengths_adversarial(codecs, R, oracle, filler, policy, force_scan):
    n, base = 130, 7
    wire, off, st, _ = oracle.encode_batch(S.mixed(n, seed=93, pmin=0, pmax=120, exotic=0.3))
    assert (st == 0).all()
    w = np.concatenate([np.full(base, 0xEE, np.uint8), np.frombuffer(wire, np.uint8)])
    T = len(w)
    lens = np.diff(off.astype(np.int64)).astype(np.uint32)
    lens[40] += 1024
    ro = np.uint64(base) + np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    why = [1 if int(a) > T else 2 if int(b) > T else 0 for a, b in zip(ro[:-1], ro[1:])]
    assert why[:41] == [0] * 41
    first1 = why.index(1)
    assert 2 in why and 0 in why[41:] and first1 > 41 and set(why[first1:]) == {1}
    pl = Placed(filler, w)
    for mode in MODES:
        want = expected(oracle, w, ro[:-1], ro[1:], why, mode)
        g, gro = run_len(R, codecs[policy, force_scan], pl, T, lens, base, mode)
        check(g, want, f"adversarial lengths scan {force_scan} mode {mode}")
        assert np.array_equal(gro, ro)                 # the true prefix sums, bad records included
        assert np.array_equal(g[2][:40], np.zeros(40, np.int32))
        for i, y in enumerate(why):
            if y:
                assert (g[2][i], g[3][i], g[4][i]) == (106, y, 0), i


# ---------------------------------------------------------------------------
# 5. body form
# ---------------------------------------------------------------------------
def _body_records(oracle, root):
    if root == L.ROOT_AUTH_UNIX_PARAMS:
        wire, off, st, _ = oracle.encode_body_batch(root, S.call_unix16(70, 40, seed=94))
        assert (st == 0).all()
        recs = _split(wire, off)
        return recs, np.array([len(x) for x in recs], np.uint32)
    recs = []
    for i in range(70):
        k = (7 * i) % 41
        recs.append(struct.pack(">I", k) + bytes([i]) * k + b"\0" * (-k % 4))
    return recs, np.full(70, 255, np.uint32)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("root", [L.ROOT_AUTH_UNIX_PARAMS, L.ROOT_OPAQUE])
def test_body_bounded(codecs, R, oracle, filler, policy, root):
    recs, param = _body_records(oracle, root)
    w, o = L.records_from_wire(recs)
    o = np.asarray(o, np.uint64)
    w = np.asarray(w, np.uint8)[:int(o[-1])]
    T = int(o[-1])
    pl = Placed(filler, w)
    codec = codecs[policy, False]
    r = o.copy()
    r[30] = o[31] + np.uint64(4)        # 30: offsets decrease (29 runs into 31)
    r[65] = T + 64                      # 64 (lane 0 of the second wave) ends past the wire
    r[66] = T + 100                     # 65 starts past it; 66: offsets decrease
    r[70] = T + 512                     # 69 ends past the wire
    why = reasons_off(r, T)
    assert {i: why[i] for i in range(70) if why[i]} == {30: 3, 64: 2, 65: 1, 66: 3, 69: 2}
    both = np.concatenate([w, filler[:PAD]])
    for mode in MODES:
        # good extents: the bounded call is the unbounded one, which is the oracle
        want = expected(oracle, w, o[:-1], o[1:], [0] * 70, mode, root, param)
        assert (want[2] == 0).all()
        gb, cb = run_body(R, codec, root, pl, T, o, mode, param)
        gu, cu = run_body(R, codec, root, pl, T, o, mode, param, bounded=False)
        check(gb, want, f"body root {root} mode {mode}")
        assert_decoded_equal(gb, gu, f"body bounded vs unbounded root {root} mode {mode}")
        assert np.array_equal(cb, want[5]) and np.array_equal(cb, cu)
        # bad extents
        want = expected(oracle, both, r[:-1], r[1:], why, mode, root, param)
        g, c = run_body(R, codec, root, pl, T, r, mode, param)
        check(g, want, f"adversarial body root {root} mode {mode}")
        assert np.array_equal(c, want[5])
        for i, y in enumerate(why):
            if y:
                assert (g[2][i], g[3][i], g[4][i], c[i]) == (106, y, 0, 0), i


# ---------------------------------------------------------------------------
# 6. mapped host wire
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("policy", POLICIES)
def test_mapped_host_wire(codecs, R, oracle, filler, policy):
    n = 100
    wire, off, st, _ = oracle.encode_batch(S.mixed(n, seed=95, pmin=0, pmax=120, exotic=0.3))
    assert (st == 0).all()
    w = np.frombuffer(wire, np.uint8)
    T = len(w)
    lens = np.diff(off.astype(np.int64)).astype(np.uint32)
    lens[60] += 1024
    ro = np.concatenate([[0], np.cumsum(lens.astype(np.uint64))]).astype(np.uint64)
    why = [1 if int(a) > T else 2 if int(b) > T else 0 for a, b in zip(ro[:-1], ro[1:])]
    assert 1 in why and 2 in why and why[:61] == [0] * 61
    codec = codecs[policy, False]
    dev = Placed(filler, w)
    host = Placed(filler, w, mapped_codec=codec, R=R)
    try:
        for mode in MODES:
            want = expected(oracle, w, ro[:-1], ro[1:], why, mode)
            gh, rh = run_len(R, codec, host, T, lens, 0, mode)
            gd, rd = run_len(R, codec, dev, T, lens, 0, mode)
            check(gh, want, f"mapped host wire mode {mode}")
            assert_decoded_equal(gh, gd, f"mapped vs device wire mode {mode}")
            assert np.array_equal(rh, ro) and np.array_equal(rd, ro)
    finally:
        host.buf.close()


# ---------------------------------------------------------------------------
# 7. C++ mirror
# ---------------------------------------------------------------------------
def test_cpp_mirror_bounded():
    """BatchDecoder::try_from with a rec_len vector whose sum exceeds
    wire_len (tests/cpp_bounded/test_bounded.cpp): the overrunning records
    are Error 106, the earlier ones decode as before."""
    exe = os.path.join(ROOT, "tests", "cpp_bounded", "test_bounded")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS test_bounded" in r.stdout
