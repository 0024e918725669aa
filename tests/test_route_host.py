"""CPU tests of onc_route_calls (decoded Calls dispatched to handlers on the
device): the symbol and its argument checks, and the arithmetic the kernels
call (onc-rpc_amd/csrc/route_plan.h) in a stand-alone host program driven over
tables and keys written here, against tests/route_model.py — keys and table
values at and above 2^31, a range ending at 2^32, both ends of a 1024-entry
table, a program with one version, the first bad entry for every table rule,
and the bin counts at every blocking of a short list."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import route_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL, RC_EALIGN = -1, -4


def test_route_symbol_and_argument_checks():
    import onc_rpc_amd.layout as L
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8 == R.ABI_VERSION      # additive: callers find the symbol by linking
    assert R.K_COUNT == 16 and len(R.K_NAMES) == 16
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and "#define ONC_K_COUNT        16" in hdr
    raw = C.CDLL(LIB)
    assert hasattr(raw, "onc_route_calls") and "onc_route_calls" in R.EXPORTED and "onc_route_calls" in hdr
    assert hasattr(R.Codec, "route_calls") and hasattr(R, "route_calls_host")
    assert L.ROUTE_DTYPE.itemsize == 24 and "typedef struct onc_route {" in hdr
    assert f"#define ONC_ROUTE_TILE {R.ROUTE_TILE}u" in hdr
    assert (R.ROUTE_TABLE_MAX, R.ROUTE_HANDLERS_MAX, R.ROUTE_ONE_HANDLER) == (M.TABLE_MAX, M.HANDLERS_MAX, M.ONE_HANDLER)
    for name in ("ONC_ROUTE_BIN_REJECTED", "ONC_ROUTE_BIN_NOT_CALL", "ONC_ROUTE_BIN_FAILED"):
        assert "#define " + name in hdr
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p, q, s = C.c_void_p(64), C.c_void_p(128), C.c_void_p(192)
    rc = lib.onc_route_calls

    # onc_route_calls(codec, msgs, status, n, table, ntab, nh, route, order, bin_first, calls_out, replies, result)
    def route(codec=fake, msgs=p, status=p, n=1, table=p, ntab=1, nh=1, route=p, order=p, bin_first=p,
              calls_out=None, replies=None, result=p, past=False):
        got = rc(codec, msgs, status, n, table, ntab, nh, route, order, bin_first, calls_out, replies, result)
        if past:                                     # got past every check other than the one added to trip it
            assert got == RC_EALIGN
        return got

    for n in (0, 1):
        # a NULL codec, result or bin_first, whatever n is
        assert route(codec=None, n=n) == RC_EINVAL
        assert route(result=None, n=n) == RC_EINVAL
        assert route(bin_first=None, n=n) == RC_EINVAL
        # the limits
        assert route(ntab=1025, n=n) == RC_EINVAL
        assert route(ntab=0xFFFFFFFF, n=n) == RC_EINVAL
        assert route(nh=254, n=n) == RC_EINVAL
        assert route(nh=0xFFFFFFFF, n=n) == RC_EINVAL
        route(ntab=1024, nh=253, n=n, result=C.c_void_p(4), past=True)
        # a table of entries needs a table
        assert route(table=None, n=n) == RC_EINVAL
        route(table=None, ntab=0, n=n, result=C.c_void_p(4), past=True)
        # alignment: the descriptors 16 bytes, bin_first and result 8, the table 4
        for a in (8, 24, 36, 17):
            assert route(msgs=C.c_void_p(a), n=n) == RC_EALIGN
            assert route(calls_out=C.c_void_p(a), n=n) == RC_EALIGN
            assert route(replies=C.c_void_p(a), n=n) == RC_EALIGN
        for a in (4, 12, 17, 20):
            assert route(bin_first=C.c_void_p(a), n=n) == RC_EALIGN
            assert route(result=C.c_void_p(a), n=n) == RC_EALIGN
        for a in (2, 5, 6, 17):
            assert route(table=C.c_void_p(a), n=n) == RC_EALIGN
        route(table=C.c_void_p(4), n=n, result=C.c_void_p(4), past=True)
    # n >= 2^32: an order entry is 32 bits
    assert route(n=1 << 32) == RC_EINVAL
    assert route(n=(1 << 64) - 1) == RC_EINVAL
    route(n=(1 << 32) - 1, result=C.c_void_p(4), past=True)
    # with records: a NULL msgs, status, route or order
    for k in ("msgs", "status", "route", "order"):
        assert route(**{k: None}) == RC_EINVAL
        route(**{k: None}, n=0, result=C.c_void_p(4), past=True)
    # a permutation cannot be done in place, and the two outputs are apart
    assert route(calls_out=p) == RC_EINVAL
    assert route(replies=p) == RC_EINVAL
    assert route(calls_out=q, replies=q) == RC_EINVAL
    route(calls_out=q, replies=s, result=C.c_void_p(4), past=True)
    # the pointer checks come before the alignment checks
    assert route(msgs=C.c_void_p(8), result=None) == RC_EINVAL
    assert route(msgs=C.c_void_p(8), order=None) == RC_EINVAL
    assert route(bin_first=C.c_void_p(4), status=None) == RC_EINVAL
    assert route(table=C.c_void_p(2), nh=254) == RC_EINVAL
    assert route(replies=C.c_void_p(8), calls_out=p) == RC_EINVAL


def _build_probe(d):
    src = os.path.join(ROOT, "tests", "cpp_route", "plan_probe.cpp")
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


def _table_cmd(rows, nh):
    return "T %d %d\n" % (len(rows), nh) + "".join("%d %d %d %d %d %d\n" % tuple(r) for r in rows)


def _check_keys(probe, rows, nh, keys):
    tab = M.table(rows)
    assert M.first_bad(tab, nh) == 0
    out = probe(_table_cmd(rows, nh) + "V\n" + "".join("K %d %d %d\n" % k for k in keys))
    assert out[0] == "V 0"
    for k, line in zip(keys, out[1:]):
        assert line == "K %d %d %d %d" % M.lookup(tab, nh, *k), (k, line)
    assert len(out) == 1 + len(keys)


def _around(rows):
    """Keys on and around every edge of every entry, and of its program and version."""
    keys = set()
    for p, v, pf, pc, _, _ in rows:
        for pp in (p - 1, p, p + 1):
            for vv in (v - 1, v, v + 1):
                for cc in (pf - 1, pf, pf + 1, pf + pc - 2, pf + pc - 1, pf + pc, 0, 0xFFFFFFFF):
                    if all(0 <= x <= 0xFFFFFFFF for x in (pp, vv, cc)):
                        keys.add((pp, vv, cc))
    return sorted(keys)


def test_probe_lookup_extremes(probe):
    H, T = 0x80000000, 0xFFFFFFFF
    # keys and table values at and above 2^31 and at 0xFFFFFFFF; a range ending exactly at 2^32; a gap;
    # ONE_HANDLER beside per-procedure ranges; a program with a single version (low == high)
    rows = [(0, 0, 0, 1, 0, 0),
            (5, 2, 0, 3, 1, 0), (5, 2, 5, 2, 4, 1), (5, 3, 0, T, 5, 1), (5, 7, H - 1, 3, 6, 0),
            (H - 1, H - 1, H - 1, 2, 9, 0), (H, H, H, 2, 11, 0), (H, T, T, 1, 13, 0),
            (T - 1, 4, 0, 1, 14, 0),
            (T, 0, 0, 1, 15, 0), (T, T, T - 3, 4, 16, 0)]
    _check_keys(probe, rows, 20, _around(rows))
    # no table: every Call is PROG_UNAVAIL, and the bin is nh
    _check_keys(probe, [], 0, [(0, 0, 0), (T, T, T), (5, 5, 5)])
    _check_keys(probe, [], 7, [(0, 0, 0)])
    # one entry
    _check_keys(probe, [(7, 7, 7, 1, 0, 1)], 1, _around([(7, 7, 7, 1, 0, 1)]))


def test_probe_lookup_1024_entries(probe):
    # 1024 entries: 64 programs x 4 versions x 4 ranges with a gap between them; the first and the last entry,
    # and every edge in between
    rows = []
    for i in range(1024):
        prog, ver, rng = 1000 + 3 * (i // 16), 1 + 2 * ((i // 4) % 4), i % 4
        rows.append((prog, ver, 10 * rng, 7, (i * 7) % 240, i & 1) if i & 1 else (prog, ver, 10 * rng, 7, i % 247, 0))
    assert len(rows) == M.TABLE_MAX
    keys = _around(rows[:3] + rows[-3:] + rows[509:515])
    rng = np.random.default_rng(7)
    for i in rng.integers(0, 1024, 300):
        p, v, pf, pc, _, _ = rows[i]
        keys.append((p + int(rng.integers(-1, 2)), v + int(rng.integers(-1, 2)), pf + int(rng.integers(0, 11))))
    _check_keys(probe, rows, 253, keys)


def test_probe_first_bad_entry(probe):
    ok = [(1, 1, 0, 2, 0, 0), (1, 1, 2, 2, 2, 0), (1, 2, 0, 4, 0, 0), (2, 0, 0, 1, 3, 0), (2, 0, 5, 1, 3, 1)]
    H, T = 0x80000000, 0xFFFFFFFF
    cases = [(ok, 4), (ok, 3), (ok, 0), ([], 0), ([(1, 1, 0, 1, 0, 0)], 0)]
    bad_rows = [(1, 1, 9, 0, 0, 0),            # proc_count == 0
                (1, 9, T, 2, 0, 1),            # proc_first + proc_count > 2^32 (wraps to 1 in 32 bits)
                (1, 9, H, H + 1, 0, 1),        # ... = 2^32 + 1
                (1, 9, 0, 1, 0, 2),            # an unknown flag
                (1, 9, 0, 1, 0, H | 1),
                (1, 9, 0, 5, 0, 0),            # handler_first + proc_count > nh
                (1, 9, 0, 1, 4, 1),            # handler_first + 1 > nh
                (1, 9, 0, 2, T, 0)]            # handler_first + proc_count wraps in 32 bits
    for row in bad_rows:
        for at in (0, 2, 4):                   # first, in the middle, last: only the entry's own rule is broken
            rows = [(10 + i, 0, 0, 1, 0, 0) for i in range(5)]
            rows[at] = (10 + at,) + row[1:]
            cases.append((rows, 4))
    good_edges = [(1, 9, T, 1, 3, 0), (1, 9, H, H, 3, 1), (1, 9, 0, T, 3, 1), (1, 9, 0, 4, 0, 0)]
    cases += [([r], 4) for r in good_edges]
    # the order rules, the bad pair first, in the middle and last
    for at in (0, 2, 3):
        for a, b in [((5, 5, 5, 1, 0, 0), (5, 5, 5, 1, 0, 0)),        # equal keys
                     ((5, 5, 5, 1, 0, 0), (5, 5, 4, 1, 0, 0)),        # out of order only in the third key word
                     ((5, 5, 5, 1, 0, 0), (5, 4, 9, 1, 0, 0)),        # ... in the second
                     ((5, 5, 5, 1, 0, 0), (4, 9, 9, 1, 0, 0)),        # ... in the first
                     ((H, 5, 5, 1, 0, 0), (H - 1, 5, 5, 1, 0, 0)),    # unsigned: 2^31 sorts after 2^31 - 1
                     ((5, 5, 5, 3, 0, 0), (5, 5, 7, 1, 0, 0)),        # the ranges overlap
                     ((5, 5, H, H, 0, 1), (5, 5, T, 1, 0, 0))]:       # ... where the first ends at 2^32
            rows = [(1, 0, 0, 1, 0, 0), (2, 0, 0, 1, 0, 0), (3, 0, 0, 1, 0, 0), (6 if at != 3 else 3, 1, 0, 1, 0, 0),
                    (7, 0, 0, 1, 0, 0)]
            rows[at], rows[at + 1] = a, b
            if at == 0:
                rows = rows[:2] + [(6, 0, 0, 1, 0, 0), (7, 0, 0, 1, 0, 0), (8, 0, 0, 1, 0, 0)]
            cases.append((rows, 4))
    # ... and such pairs in order
    cases.append(([(1, 0, 0, 1, 0, 0), (5, 5, 5, 3, 0, 0), (5, 5, 8, 1, 0, 0), (H - 1, 5, 5, 1, 0, 0),
                   (H, 5, 5, 1, 0, 0)], 4))
    # two bad entries: the first is reported; an entry's own rule comes with the entry, its pair's too
    cases.append(([(5, 5, 5, 0, 0, 0), (1, 1, 1, 0, 0, 0)], 4))
    cases.append(([(1, 0, 0, 1, 0, 0), (5, 5, 5, 1, 0, 0), (5, 5, 5, 0, 0, 0)], 4))
    script = "".join(_table_cmd(rows, nh) + "V\n" for rows, nh in cases)
    out = probe(script)
    want = [M.first_bad(M.table(rows), nh) for rows, nh in cases]
    assert out == ["V %d" % w for w in want]
    assert want[:5] == [0, 2, 1, 0, 1]
    assert 0 in want and {1, 2, 3, 4, 5} <= set(want)


def test_probe_bin_counts_at_every_blocking(probe):
    nh = 3
    rng = np.random.default_rng(3)
    lists = [[], [5], [0], [5, 0], [0, 5, 0, 5, 0, 5, 0], list(range(5, -1, -1)) * 2, [2] * 9,
             [5] + [0] * 8, [int(x) for x in rng.integers(0, 6, 13)]]
    script, want = _table_cmd([], nh), []
    for bins in lists:
        order = np.argsort(np.array(bins, np.int64), kind="stable")
        first = np.concatenate([[0], np.cumsum(np.bincount(np.array(bins, np.int64), minlength=nh + 3))])
        for tile in range(1, len(bins) + 3):
            script += "B %d %d %s\n" % (tile, len(bins), " ".join(map(str, bins)))
            want.append(("B " + " ".join(map(str, order))).rstrip() + " | " + " ".join(map(str, first)))
    assert probe(script) == want


def test_cpp_mirror_program_compiles():
    """RouteTable, route_calls and RoutedCalls (include/onc_rpc.hpp) build
    against the C ABI (build() compiles tests/cpp_route)."""
    exe = os.path.join(ROOT, "tests", "cpp_route", "test_route")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "include", "onc_rpc.hpp")).read()
    assert "onc_route_calls" in hpp and "RouteTable" in hpp and "RoutedCalls" in hpp and "reject_replies" in hpp
