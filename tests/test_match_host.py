"""CPU tests of onc_match_replies (decoded Replies paired with pending Calls on
the device): the symbol and its argument checks, and the arithmetic the
kernels call (onc-rpc_amd/csrc/match_plan.h) in a stand-alone host program
driven from here against tests/match_model.py — the slot count around every
power of two and at the largest list, the wrap of the next slot, the scratch
words formed in 64 bits, and a lane-by-lane emulation of insert and probe on
lists with repeats, with and without the one-chain hash, in three insertion
orders. The program is also built with the address and undefined-behaviour
sanitizers and run stand-alone."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import match_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL, RC_EALIGN = -1, -4


def test_match_symbol_and_argument_checks():
    import onc_rpc_amd.layout as L
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8 == R.ABI_VERSION      # additive: callers find the symbol by linking
    assert R.K_COUNT == 16 and len(R.K_NAMES) == 16
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and "#define ONC_K_COUNT        16" in hdr
    raw = C.CDLL(LIB)
    assert hasattr(raw, "onc_match_replies") and "onc_match_replies" in R.EXPORTED and "onc_match_replies" in hdr
    assert hasattr(R.Codec, "match_replies") and hasattr(R, "match_replies_host")
    assert L.PENDING_DTYPE.itemsize == 16 and "typedef struct onc_pending {" in hdr
    assert [L.PENDING_DTYPE.fields[k][1] for k in ("conn", "xid", "tag")] == [0, 4, 8]
    for name, value in (("UNKNOWN", R.MATCH_UNKNOWN), ("DUPLICATE", R.MATCH_DUPLICATE),
                        ("NOT_REPLY", R.MATCH_NOT_REPLY), ("FAILED", R.MATCH_FAILED), ("NONE", R.MATCH_NONE),
                        ("MAX", R.MATCH_MAX)):
        line = [ln for ln in hdr.split("\n") if ln.startswith("#define ONC_MATCH_" + name + " ")]
        assert len(line) == 1 and line[0].split()[2] == "0x%08Xu" % value, (name, line)
    assert f"#define ONC_MATCH_TILE      {R.MATCH_TILE}u" in hdr
    assert "#define ONC_VARIANT_MATCH_ONE_CHAIN  0x%xu" % R.VARIANT_MATCH_ONE_CHAIN in hdr
    assert (R.MATCH_UNKNOWN, R.MATCH_DUPLICATE, R.MATCH_NOT_REPLY, R.MATCH_FAILED, R.MATCH_NONE, R.MATCH_MAX,
            R.MATCH_TILE, R.VARIANT_MATCH_ONE_CHAIN) == (M.UNKNOWN, M.DUPLICATE, M.NOT_REPLY, M.FAILED, M.NONE, M.MAX,
                                                        M.TILE, M.ONE_CHAIN)
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p, q = C.c_void_p(64), C.c_void_p(128)
    bad8 = C.c_void_p(4)                             # a result that passes every check but its own alignment
    rc = lib.onc_match_replies

    # onc_match_replies(codec, msgs, status, rec_conn, n, pending, np, match, hit, tag_out, still, result)
    def match(codec=fake, msgs=p, status=p, rec_conn=None, n=1, pending=p, np_=1, match=p, hit=p, tag_out=None,
              still=None, result=p, past=False):
        got = rc(codec, msgs, status, rec_conn, n, pending, np_, match, hit, tag_out, still, result)
        if past:                                     # got past every check other than the one added to trip it
            assert got == RC_EALIGN
        return got

    for n in (0, 1):
        for np_ in (0, 1):
            # a NULL codec or result, whatever n and np are
            assert match(codec=None, n=n, np_=np_) == RC_EINVAL
            assert match(result=None, n=n, np_=np_) == RC_EINVAL
            match(n=n, np_=np_, result=bad8, past=True)
            # alignment: descriptors, list and still 16 bytes; tag_out and result 8; the word arrays 4
            for a in (8, 24, 36, 17):
                assert match(msgs=C.c_void_p(a), n=n, np_=np_) == RC_EALIGN
                assert match(pending=C.c_void_p(a), n=n, np_=np_) == RC_EALIGN
                assert match(still=C.c_void_p(a), n=n, np_=np_) == RC_EALIGN
            for a in (4, 12, 17, 20):
                assert match(tag_out=C.c_void_p(a), n=n, np_=np_) == RC_EALIGN
                assert match(result=C.c_void_p(a), n=n, np_=np_) == RC_EALIGN
            for a in (2, 5, 6, 17):
                for k in ("rec_conn", "match", "hit", "status"):
                    assert match(**{k: C.c_void_p(a)}, n=n, np_=np_) == RC_EALIGN
            match(rec_conn=C.c_void_p(4), match=C.c_void_p(12), hit=C.c_void_p(20), status=C.c_void_p(28),
                  tag_out=C.c_void_p(8), still=C.c_void_p(16), n=n, np_=np_, result=bad8, past=True)
            # the compaction is not done in place
            assert match(still=p, n=n, np_=np_) == RC_EINVAL
            match(still=q, n=n, np_=np_, result=bad8, past=True)
    # n or np >= ONC_MATCH_MAX
    for big in (M.MAX, M.MAX + 1, 1 << 32, (1 << 64) - 1):
        assert match(n=big) == RC_EINVAL
        assert match(np_=big) == RC_EINVAL
    match(n=M.MAX - 1, np_=M.MAX - 1, result=bad8, past=True)
    # with records: a NULL msgs, status or match; with entries: a NULL pending or hit
    for k in ("msgs", "status", "match"):
        assert match(**{k: None}) == RC_EINVAL
        assert match(**{k: None}, np_=0) == RC_EINVAL
        match(**{k: None}, n=0, result=bad8, past=True)
    for k in ("pending", "hit"):
        assert match(**{k: None}) == RC_EINVAL
        assert match(**{k: None}, n=0) == RC_EINVAL
        match(**{k: None}, np_=0, result=bad8, past=True)
    # rec_conn, tag_out and still are optional
    match(rec_conn=None, tag_out=None, still=None, result=bad8, past=True)
    # the pointer checks come before the alignment checks
    assert match(msgs=C.c_void_p(8), result=None) == RC_EINVAL
    assert match(msgs=C.c_void_p(8), match=None) == RC_EINVAL
    assert match(tag_out=C.c_void_p(4), hit=None) == RC_EINVAL
    assert match(hit=C.c_void_p(2), n=M.MAX) == RC_EINVAL
    assert match(status=C.c_void_p(2), still=p) == RC_EINVAL


def _build_probe(d):
    src = os.path.join(ROOT, "tests", "cpp_match", "plan_probe.cpp")
    inc = os.path.join(ROOT, "onc-rpc_amd", "csrc")
    plain, san = os.path.join(d, "plan_probe"), os.path.join(d, "plan_probe_san")
    base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, src, "-o"]
    subprocess.run(base + [plain], check=True, capture_output=True, text=True)
    r = subprocess.run(base + [san, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                       capture_output=True, text=True)
    return [plain] + ([san] if r.returncode == 0 else [])       # (no sanitizer runtime here: the plain build alone)


@pytest.fixture(scope="module")
def probe():
    with tempfile.TemporaryDirectory() as d:
        exes = _build_probe(d)

        def run(script):
            outs = []
            for exe in exes:
                r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=120)
                assert r.returncode == 0, (exe, r.stdout[-2000:], r.stderr[-2000:])
                outs.append(r.stdout.split("\n")[:-1])
            assert all(o == outs[0] for o in outs)
            return outs[0]
        yield run


def _slots(np_):
    """The least power of two >= 2 np, and >= 16."""
    s = 16
    while s < 2 * np_:
        s *= 2
    return s


def test_probe_slot_count(probe):
    nps = {0, 1, 2, 7, 8, 9, M.MAX - 1}
    for k in range(1, 32):
        nps |= {2**k - 1, 2**k, 2**k + 1}
    nps = sorted(x for x in nps if x < M.MAX)
    out = probe("".join("S %d\n" % x for x in nps))
    assert out == ["S %d" % _slots(x) for x in nps]
    assert _slots(0) == 16 and _slots(8) == 16 and _slots(9) == 32 and _slots(M.MAX - 1) == 1 << 33
    assert all(_slots(x) >= 2 * x and _slots(x) < max(4 * x, 17) for x in nps)


def test_probe_next_slot_wraps(probe):
    cases = [(0, 16), (14, 16), (15, 16), (1023, 1024), (2**33 - 2, 2**33), (2**33 - 1, 2**33), (2**32 - 1, 2**33),
             (2**32, 2**33)]
    out = probe("".join("N %d %d\n" % c for c in cases))
    assert out == ["N %d" % ((s + 1) % S) for s, S in cases]
    assert out[2] == "N 0" and out[5] == "N 0" and out[6] == "N %d" % 2**32


def test_probe_scratch_words_in_64_bits(probe):
    T = M.TILE
    cases = [(0, 0), (1, 1), (T, T), (T + 1, T + 1), (5, 0), (0, 5), (3 * T + 1, 2), (1 << 20, 1 << 20),
             (1 << 20, 1 << 22), (M.MAX - 1, M.MAX - 1), (0, M.MAX - 1), (M.MAX - 1, 0), (1 << 31, (1 << 31) + 1)]
    out = probe("".join("W %d %d\n" % c for c in cases))
    for (n, np_), line in zip(cases, out):
        S, rt, pt = _slots(np_), -(-n // T), -(-np_ // T)
        clear = S + (np_ + 3) // 4 * 4
        assert line == "W %d %d %d %d %d %d %d %d" % (S, S, clear, clear, clear + 5 * rt, clear + 5 * rt + pt, rt, pt), \
            (n, np_, line)
        # the contract: under 32 bytes per pending entry plus under 1 byte per 32 records (and a constant)
        words = clear + 5 * rt + pt
        assert 4 * words <= 32 * np_ + n // 32 + 128, (n, np_)
    assert int(out[9].split()[6]) > 1 << 33                      # (the largest call's words do not fit 32 bits)
    # a tile's class counts lie class-major
    cc = [(0, 0, 1), (4, 0, 1), (1, 5, 7), (4, 6, 7), (4, (1 << 22) - 1, 1 << 22), (4, 4194303, 4194304)]
    assert probe("".join("C %d %d %d\n" % c for c in cc)) == ["C %d" % (c * rt + t) for c, t, rt in cc]
    # a final match[] value's place in result
    rr = [(0, 0), (1, 0), (M.MAX - 1, 0), (M.UNKNOWN, 1), (M.DUPLICATE, 2), (M.NOT_REPLY, 3), (M.FAILED, 4)]
    assert probe("".join("R %d\n" % m for m, _ in rr)) == ["R %d" % c for _, c in rr]


def test_probe_hash_in_range_and_one_chain(probe):
    rng = np.random.default_rng(5)
    keys = [(0, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (0xFFFFFFFF, 0), (1, 2), (2, 1)]
    keys += [(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, (50, 2))]
    for S in (16, 1024, 1 << 33):
        out = probe("".join("H %d %d %d 0\nH %d %d %d %d\n" % (c, x, S, c, x, S, M.ONE_CHAIN) for c, x in keys))
        plain, chain = [int(v.split()[1]) for v in out[0::2]], [int(v.split()[1]) for v in out[1::2]]
        assert all(0 <= h < S for h in plain) and chain == [S - 2] * len(keys)
        assert len(set(plain)) > (4 if S == 16 else 40)          # it spreads; and both words enter it:
    out = probe("".join("H %d %d %d 0\n" % (c, x, 1 << 33) for c, x in ((1, 2), (2, 1), (1, 3), (2, 2))))
    assert len(set(out)) == 4
    # xids counting up on connections counting up: no slot of 4x as many takes more than a few
    S = 1 << 14
    out = probe("".join("H %d %d %d 0\n" % (c, 1000 + x, S) for c in range(64) for x in range(64)))
    assert max(np.bincount([int(v.split()[1]) for v in out], minlength=S)) <= 6


def _emulate(probe, rows, recs):
    want = []
    lead = M.leads(M.pending([(c, x, 0) for c, x in rows]))
    for k in recs:
        want.append(lead.get(k, -1))
    script = ""
    for var in (0, M.ONE_CHAIN):
        for order in (0, 1, 2):
            script += "E %d %d %d %d\n" % (var, order, len(rows), len(recs))
            script += "".join("%d %d\n" % k for k in rows) + "".join("%d %d\n" % k for k in recs)
    out = probe(script)
    assert out == [("E " + " ".join(map(str, want))).rstrip()] * 6
    return want


def test_probe_insert_and_probe_emulation(probe):
    TOP = 0xFFFFFFFF
    # no list; one entry; the reserved-looking keys; keys that differ in one word only, and swapped
    assert _emulate(probe, [], [(0, 0), (TOP, TOP)]) == [-1, -1]
    assert _emulate(probe, [(3, 4)], [(3, 4), (4, 3), (3, 5)]) == [0, -1, -1]
    rows = [(TOP, TOP), (0, 0), (0, TOP), (TOP, 0), (1, 2), (2, 1), (1, 1), (2, 2), (0x80000000, 0x7FFFFFFF),
            (0x7FFFFFFF, 0x80000000)]
    assert _emulate(probe, rows, rows + [(5, 5), (0, 1)]) == list(range(10)) + [-1, -1]
    # repeats: a key three times among others; every entry the same key; the lead is the lowest index
    rows = [(1, 1), (7, 9), (2, 2), (7, 9), (3, 3), (7, 9), (1, 1)]
    assert _emulate(probe, rows, [(7, 9), (1, 1), (2, 2), (3, 3), (9, 7)]) == [1, 0, 2, 4, -1]
    assert _emulate(probe, [(6, 6)] * 40, [(6, 6), (6, 7)]) == [0, -1]
    # a list that fills half of its table exactly (np = 2^k), and one over (the table doubles)
    rng = np.random.default_rng(11)
    for np_ in (8, 9, 64, 65, 300):
        keys = [(int(c), int(x)) for c, x in rng.integers(0, 6, (np_, 2))]     # few keys: many repeats
        recs = [(c, x) for c in range(7) for x in range(7)]
        want = _emulate(probe, keys, recs)
        assert -1 in want and max(want) >= 0
        keys = [(int(c), int(x)) for c, x in rng.integers(0, 1 << 32, (np_, 2))]
        _emulate(probe, keys, keys[::3] + [(1, 1)])


def test_cpp_mirror_program_compiles():
    """PendingCalls, match_replies and MatchedReplies (include/onc_rpc.hpp)
    build against the C ABI (build() compiles tests/cpp_match)."""
    exe = os.path.join(ROOT, "tests", "cpp_match", "test_match")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "include", "onc_rpc.hpp")).read()
    assert "onc_match_replies" in hpp and "PendingCalls" in hpp and "MatchedReplies" in hpp and "answered" in hpp
