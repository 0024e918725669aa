"""CPU tests of onc_group_by_conn and onc_conn_extents (a send batch grouped by
connection on the device): the symbols and their argument checks, and the
arithmetic the kernels call (onc-rpc_amd/csrc/group_plan.h) in a stand-alone
host program driven over lists written here, against tests/group_model.py —
bits and passes on either side of every change in pass count, the digits of a
key, the sort of a short list at every tile size driven pass by pass, and the
scratch size at the largest batch."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import group_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL, RC_EALIGN = -1, -4


def test_group_symbols_and_abi_kept():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8 == R.ABI_VERSION      # additive: callers find the symbols by linking
    assert R.K_COUNT == 16 and len(R.K_NAMES) == 16
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and "#define ONC_K_COUNT        16" in hdr
    assert lib.onc_status_str(107) == b"unknown status"      # no status code was added
    raw = C.CDLL(LIB)
    for name in ("onc_group_by_conn", "onc_conn_extents"):
        assert hasattr(raw, name) and name in R.EXPORTED and name in hdr
    assert hasattr(R.Codec, "group_by_conn") and hasattr(R.Codec, "conn_extents")
    assert hasattr(R, "group_by_conn_host") and hasattr(R, "conn_extents_host")
    assert f"#define ONC_GROUP_TILE     {R.GROUP_TILE}u" in hdr and R.GROUP_TILE == M.TILE
    assert "#define ONC_GROUP_CONN_MAX 0x00FFFFFFu" in hdr and R.GROUP_CONN_MAX == M.CONN_MAX == (1 << 24) - 1


def test_group_by_conn_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p, q, s, t = C.c_void_p(64), C.c_void_p(128), C.c_void_p(192), C.c_void_p(256)
    bad8 = C.c_void_p(4)                             # a result that trips the last check there is
    rc = lib.onc_group_by_conn

    # onc_group_by_conn(codec, rec_conn, nsrc, via, n, nconn, order, conn_first, msgs, msgs_out, result)
    def group(codec=fake, rec_conn=p, nsrc=1, via=None, n=1, nconn=1, order=q, conn_first=s, msgs=None,
              msgs_out=None, result=t, past=False):
        got = rc(codec, rec_conn, nsrc, via, n, nconn, order, conn_first, msgs, msgs_out, result)
        if past:                                     # got past every check other than the one added to trip it
            assert got == RC_EALIGN
        return got

    for n in (0, 1):
        # a NULL codec, result or conn_first, whatever n is
        assert group(codec=None, n=n, nsrc=n) == RC_EINVAL
        assert group(result=None, n=n, nsrc=n) == RC_EINVAL
        assert group(conn_first=None, n=n, nsrc=n) == RC_EINVAL
        # the limit of nconn
        assert group(nconn=1 << 24, n=n, nsrc=n) == RC_EINVAL
        assert group(nconn=0xFFFFFFFF, n=n, nsrc=n) == RC_EINVAL
        group(nconn=(1 << 24) - 1, n=n, nsrc=n, result=bad8, past=True)
        group(nconn=0, n=n, nsrc=n, result=bad8, past=True)
        # without via the items are rec_conn's entries
        assert group(n=n, nsrc=n + 1) == RC_EINVAL
        assert group(n=n + 1, nsrc=n) == RC_EINVAL
        group(via=p, order=q, n=n, nsrc=n + 5, result=bad8, past=True)
        group(via=p, order=q, n=n, nsrc=0, rec_conn=None, result=bad8, past=True)
        # descriptors: msgs_out needs msgs, and somewhere else
        assert group(msgs_out=p, n=n, nsrc=n) == RC_EINVAL
        assert group(msgs=p, msgs_out=p, n=n, nsrc=n) == RC_EINVAL
        group(msgs=p, msgs_out=q, n=n, nsrc=n, result=bad8, past=True)
        group(msgs=p, n=n, nsrc=n, result=bad8, past=True)
        # alignment: the descriptors 16 bytes, conn_first and result 8, the word arrays 4
        for a in (8, 24, 36, 17):
            assert group(msgs=C.c_void_p(a), n=n, nsrc=n) == RC_EALIGN
            assert group(msgs=p, msgs_out=C.c_void_p(a), n=n, nsrc=n) == RC_EALIGN
        for a in (4, 12, 17, 20):
            assert group(conn_first=C.c_void_p(a), n=n, nsrc=n) == RC_EALIGN
            assert group(result=C.c_void_p(a), n=n, nsrc=n) == RC_EALIGN
        for a in (2, 5, 6, 17):
            assert group(rec_conn=C.c_void_p(a), n=n, nsrc=n) == RC_EALIGN
            assert group(via=C.c_void_p(a), n=n, nsrc=n) == RC_EALIGN
            assert group(order=C.c_void_p(a), n=n, nsrc=n) == RC_EALIGN
    # n >= 2^32: an order entry is 32 bits
    assert group(n=1 << 32, nsrc=1 << 32) == RC_EINVAL
    assert group(n=(1 << 64) - 1, nsrc=(1 << 64) - 1) == RC_EINVAL
    assert group(via=p, n=1 << 32) == RC_EINVAL
    group(n=(1 << 32) - 1, nsrc=(1 << 32) - 1, result=bad8, past=True)
    # with items: a NULL order; with items and sources: a NULL rec_conn
    assert group(order=None) == RC_EINVAL
    group(order=None, n=0, nsrc=0, result=bad8, past=True)
    assert group(rec_conn=None) == RC_EINVAL
    assert group(rec_conn=None, via=p, nsrc=3) == RC_EINVAL
    group(rec_conn=None, n=0, nsrc=0, result=bad8, past=True)
    group(rec_conn=None, via=p, n=0, nsrc=7, result=bad8, past=True)
    # a permutation cannot be done in place
    assert group(via=p, order=p) == RC_EINVAL
    group(via=p, order=q, result=bad8, past=True)
    # the pointer checks come before the alignment checks
    assert group(msgs=C.c_void_p(8), result=None) == RC_EINVAL
    assert group(msgs=C.c_void_p(8), order=None) == RC_EINVAL
    assert group(conn_first=C.c_void_p(4), rec_conn=None) == RC_EINVAL
    assert group(order=C.c_void_p(2), nconn=1 << 24) == RC_EINVAL
    assert group(rec_conn=C.c_void_p(2), n=2) == RC_EINVAL
    assert group(msgs_out=C.c_void_p(8)) == RC_EINVAL
    assert group(via=C.c_void_p(2), order=C.c_void_p(2)) == RC_EINVAL


def test_conn_extents_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    fake, p, q, s = C.c_void_p(8), C.c_void_p(64), C.c_void_p(128), C.c_void_p(192)
    rc = lib.onc_conn_extents

    # onc_conn_extents(codec, rec_off, nrec, conn_first, nconn, conn_off)
    def ext(codec=fake, rec_off=p, nrec=1, conn_first=q, nconn=1, conn_off=s):
        return rc(codec, rec_off, nrec, conn_first, nconn, conn_off)

    for nrec in (0, 1, (1 << 64) - 1):
        assert ext(codec=None, nrec=nrec) == RC_EINVAL
        assert ext(rec_off=None, nrec=nrec) == RC_EINVAL
        assert ext(conn_first=None, nrec=nrec) == RC_EINVAL
        assert ext(conn_off=None, nrec=nrec) == RC_EINVAL
        assert ext(nconn=1 << 24, nrec=nrec) == RC_EINVAL
        assert ext(nconn=0xFFFFFFFF, nrec=nrec) == RC_EINVAL
        for a in (4, 12, 17, 20):
            assert ext(rec_off=C.c_void_p(a), nrec=nrec) == RC_EALIGN
            assert ext(conn_first=C.c_void_p(a), nrec=nrec) == RC_EALIGN
            assert ext(conn_off=C.c_void_p(a), nrec=nrec) == RC_EALIGN
        # the largest nconn gets past the limit
        assert ext(nconn=(1 << 24) - 1, conn_off=C.c_void_p(4), nrec=nrec) == RC_EALIGN
    # pointers before alignment
    assert ext(rec_off=C.c_void_p(4), conn_off=None) == RC_EINVAL
    assert ext(conn_first=C.c_void_p(4), nconn=1 << 24) == RC_EINVAL


def _build_probe(d):
    src = os.path.join(ROOT, "tests", "cpp_group", "plan_probe.cpp")
    inc = os.path.join(ROOT, "onc-rpc_amd", "csrc")
    plain, san = os.path.join(d, "plan_probe"), os.path.join(d, "plan_probe_ubsan")
    base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, src, "-o"]
    subprocess.run(base + [plain], check=True, capture_output=True, text=True)
    r = subprocess.run(base + [san, "-fsanitize=undefined", "-fno-sanitize-recover=undefined"], capture_output=True,
                       text=True)
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


NCONNS = (0, 1, 2, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1)


def test_probe_bits_and_passes(probe):
    out = probe("".join("P %d\n" % c for c in NCONNS))
    assert out == ["P %d %d" % (M.bits(c), M.passes(c)) for c in NCONNS]
    assert [M.passes(c) for c in NCONNS] == [0, 1, 1, 1, 2, 2, 2, 3, 3, 3]


def test_probe_digits_reassemble_the_clamped_key(probe):
    rng = np.random.default_rng(5)
    cases = []
    for nconn in NCONNS:
        conns = {0, 1, 255, 256, 0xFF00, 0x10000, 0xABCDEF, 0x80000000, 0xFFFFFFFF, nconn, max(nconn - 1, 0), nconn + 1}
        conns |= {int(x) for x in rng.integers(0, nconn + 2, 6)}
        cases += [(nconn, c) for c in sorted(conns)]
    out = probe("".join("D %d %d\n" % c for c in cases))
    assert len(out) == len(cases)
    for (nconn, conn), line in zip(cases, out):
        words = [int(x) for x in line.split()[1:]]
        key, digits = words[0], words[1:]
        assert key == min(conn, nconn)
        assert len(digits) == M.passes(nconn) and all(0 <= d < 256 for d in digits)
        assert sum(d << (8 * p) for p, d in enumerate(digits)) == key, (nconn, conn, line)


def _sort_cmd(tile, nconn, rec_conn, via):
    return "S %d %d %d %d %s %s\n" % (tile, nconn, len(rec_conn), 0 if via is None else len(via),
                                      " ".join(map(str, rec_conn)), "" if via is None else " ".join(map(str, via)))


def test_probe_sort_at_every_tile_size(probe):
    rng = np.random.default_rng(9)
    T = 0xFFFFFFFF
    cases = [(300, [], None), (300, [5], None), (300, [299, 0], None),
             (70000, [69999, 256, 0, 65536, 256, 0, 69999, 1, 65536, 257, 1], None),       # three passes
             (70000, [0x10001, 0x00001] * 5, None),                # two keys apart only in the top digit
             (70000, [0x00101, 0x00001] * 5, None),                # ... in the middle digit
             (70000, [0x00002, 0x00001] * 5, None),                # ... in the low digit
             (300, [299, 300, 301, T, 0, 299, T, 0, 300], None),   # the edges of the clamp
             (300, [int(x) for x in rng.integers(0, 302, 13)], None),
             (0, [7, 0, T, 3], None),                              # no pass: the identity
             (1, [1, 0, 1, 0, 0, 2, 0], None),
             (300, [10, 299, 10, 5], [3, 3, 0, 4, 1, 5, T, 2, 0]),             # via: repeats, entries at and past nsrc
             (70000, [int(x) for x in rng.integers(0, 70002, 9)], [int(x) for x in rng.integers(0, 11, 12)])]
    script, want = "", []
    for nconn, rc, via in cases:
        m = M.group(rc, via, nconn)
        n = len(m["order"])
        for tile in range(1, n + 3):
            script += _sort_cmd(tile, nconn, rc, via)
            want.append(("S " + " ".join(map(str, m["order"]))).rstrip() + " | " + " ".join(map(str, m["conn_first"]))
                        + " | " + " ".join(map(str, m["result"])))
    assert probe(script) == want


def test_probe_scratch_size_is_formed_in_64_bits(probe):
    ns = [0, 1, 1023, 1024, 1025, 65536, (1 << 31) + 5, (1 << 32) - 1]
    out = probe("".join("Z %d\n" % n for n in ns))
    got = [int(line.split()[1]) for line in out]
    for n, b in zip(ns, got):
        tiles = (n + 1023) // 1024
        assert b >= 16 * n + 4 * 256 * tiles                       # two (key, index) buffers and the counts
        assert b <= 17 * n + 7216
    assert got[-1] > 1 << 36 and got[-1] < 28 * ((1 << 32) - 1)    # 64-bit, and under onc_defragment's 28 bytes an item
    # under the buffer onc_codec_reserve(n) leaves, whose floor is 65536 fragments' worth
    for n, b in zip(ns, got):
        assert b < 28 * max(n, 65536)


def test_cpp_mirror_program_compiles():
    """group_by_conn and GroupedSends (include/onc_rpc.hpp) build against the
    C ABI (build() compiles tests/cpp_group)."""
    exe = os.path.join(ROOT, "tests", "cpp_group", "test_group")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "include", "onc_rpc.hpp")).read()
    for word in ("onc_group_by_conn", "onc_conn_extents", "GroupedSends", "connection_streams", "dropped()", "active()"):
        assert word in hpp
