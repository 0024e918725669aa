"""CPU tests of onc_xdr_unpack (Call arguments decoded into columns on the
device): the symbols, constants and argument checks, onc_xdr_schema_check for
the first bad field under every rule, and the arithmetic the kernel calls
(onc-rpc_amd/csrc/xdr_plan.h) in a stand-alone host program built with
-fsanitize=address,undefined and driven over schemas and payloads written
here, against tests/xdr_model.py — every type with 0 .. 12 bytes left, length
words at and past their maximum and where pad4 reaches 2^32, counts whose
32-bit byte product is 0, and base + L at 0xFFFFFFFF and 2^32."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import xdr_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL, RC_EALIGN = -1, -4
T = 0xFFFFFFFF


def test_xdr_symbols_and_constants():
    import onc_rpc_amd.layout as L
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8 == R.ABI_VERSION      # additive: callers find the symbols by linking
    assert R.K_COUNT == 16 and len(R.K_NAMES) == 16
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and "#define ONC_K_COUNT        16" in hdr
    raw = C.CDLL(LIB)
    for name in ("onc_xdr_unpack", "onc_xdr_schema_check"):
        assert hasattr(raw, name) and name in R.EXPORTED and name in hdr
    assert hasattr(R.Codec, "xdr_unpack") and hasattr(R, "xdr_unpack_host")
    assert L.XDR_FIELD_DTYPE.itemsize == 24 and "typedef struct onc_xdr_field {" in hdr
    assert f"#define ONC_XDR_TILE {R.XDR_TILE}u" in hdr and f"#define ONC_XDR_FIELDS_MAX {R.XDR_FIELDS_MAX}u" in hdr
    assert R.XDR_FIELDS_MAX == M.FIELDS_MAX

    def define(name):
        import re
        m = re.search(r"#define %s\s+(0x[0-9A-Fa-f]+|\d+)u" % name, hdr)
        assert m, name
        return int(m.group(1), 0)
    for names, mod in ((("U32", "U64", "BOOL", "OPAQUE_FIXED", "OPAQUE_VAR", "ARRAY32", "ARRAY64", "SELECT", "IF",
                         "NO_COLUMN", "EXACT", "OK", "SKIPPED", "BAD_EXTENT", "SHORT", "BAD_BOOL", "TOO_LONG", "TRAILING",
                         "HEAD_SHORT"), None),):
        for nm in names:
            assert define("ONC_XDR_" + nm) == getattr(M, nm) == getattr(R, "XDR_" + nm), nm
    assert [getattr(M, k) for k in ("OK", "SKIPPED", "BAD_EXTENT", "SHORT", "BAD_BOOL", "TOO_LONG", "TRAILING",
                                    "HEAD_SHORT")] == list(range(8))
    assert define("ONC_ACCEPT_GARBAGE_ARGS") == M.ACCEPT_GARBAGE_ARGS


def _fields(rows):
    import onc_rpc_amd.layout as L
    f = np.zeros(len(rows), L.XDR_FIELD_DTYPE)
    for i, r in enumerate(rows):
        r = tuple(r) + (0,) * (5 - len(r))
        f[i] = r
    return f


def test_xdr_unpack_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p = C.c_void_p(64)
    good = _fields([(M.U32, 0, 0), (M.U64, 0, 16), (M.U32 | M.NO_COLUMN,)])
    fn = lib.onc_xdr_unpack

    # onc_xdr_unpack(codec, wire, wire_len, msgs, status, n, rec_start, head_len, fields, nf, flags, cols, cols_cap,
    #                xstat, present, rest_pos, rest_len, replies, result)
    def call(codec=fake, wire=p, wire_len=1 << 20, msgs=p, status=p, n=1, rec_start=None, head_len=0, fields=good,
             nf=None, flags=0, cols=p, cols_cap=64, xstat=p, present=None, rest_pos=None, rest_len=None, replies=None,
             result=p, past=False):
        fp = None if fields is None else C.c_void_p(fields.ctypes.data)
        nf = (0 if fields is None else len(fields)) if nf is None else nf
        got = fn(codec, wire, wire_len, msgs, status, n, rec_start, head_len, fp, nf, flags, cols, cols_cap, xstat,
                 present, rest_pos, rest_len, replies, result)
        if past:                                     # got past every check other than the one added to trip it
            assert got == RC_EALIGN
        return got

    trip = dict(result=C.c_void_p(4), past=True)
    for n in (0, 1):
        assert call(codec=None, n=n) == RC_EINVAL
        assert call(result=None, n=n) == RC_EINVAL
        call(n=n, **trip)
        # a bad schema: a rule of a field, more than 64 fields, a NULL schema with fields
        assert call(fields=_fields([(7,)]), n=n) == RC_EINVAL
        assert call(fields=_fields([(M.U32, 0, 0), (M.U32, 0, 2)]), n=n) == RC_EINVAL
        assert call(fields=_fields([(M.U32 | M.NO_COLUMN,)] * 65), n=n) == RC_EINVAL
        assert call(fields=None, nf=1, n=n) == RC_EINVAL
        call(fields=_fields([(M.U32 | M.NO_COLUMN,)] * 64), n=n, **trip)
        call(fields=None, nf=0, cols=None, cols_cap=0, n=n, **trip)
        # unknown call flags
        for fl in (2, 4, 0x80000000, 3):
            assert call(flags=fl, n=n) == RC_EINVAL
        call(flags=M.EXACT, n=n, **trip)
        # both position forms at once; a head_len onc_decode_heads would refuse
        assert call(rec_start=p, head_len=64, n=n) == RC_EINVAL
        for hl in (16, 48, 63, 65, 72, 4112, 8192, T):
            assert call(head_len=hl, n=n) == RC_EINVAL
        call(head_len=64, n=n, **trip)
        call(head_len=4096, n=n, **trip)
        call(rec_start=p, n=n, **trip)
        # one of rest_pos / rest_len without the other
        assert call(rest_pos=p, n=n) == RC_EINVAL
        assert call(rest_len=p, n=n) == RC_EINVAL
        call(rest_pos=p, rest_len=p, n=n, **trip)
        # a NULL cols when some field has a column
        assert call(cols=None, n=n) == RC_EINVAL
        call(cols=None, fields=_fields([(M.U32 | M.NO_COLUMN,)]), n=n, **trip)
        # alignment: descriptors 16 bytes; cols, present and result 8
        for a in (8, 24, 36, 17):
            assert call(msgs=C.c_void_p(a), n=n) == RC_EALIGN
            assert call(replies=C.c_void_p(a), n=n) == RC_EALIGN
        for a in (4, 12, 17, 20):
            assert call(cols=C.c_void_p(a), n=n) == RC_EALIGN
            assert call(present=C.c_void_p(a), n=n) == RC_EALIGN
            assert call(result=C.c_void_p(a), n=n) == RC_EALIGN
    # the heads form: wire_len < n * head_len (the product is not formed in 64 bits either)
    assert call(head_len=64, n=3, wire_len=191, cols_cap=1 << 20) == RC_EINVAL
    call(head_len=64, n=3, wire_len=192, cols_cap=1 << 20, **trip)
    assert call(head_len=4096, n=1 << 62, wire_len=(1 << 64) - 1, fields=_fields([(M.U32 | M.NO_COLUMN,)])) == RC_EINVAL
    # the columns of n records must fit cols_cap
    assert call(n=2, cols_cap=31) == RC_EINVAL        # the u64 column at 16 takes 16 bytes
    call(n=2, cols_cap=32, **trip)
    call(n=4, cols_cap=1 << 20, **trip)
    assert call(n=5, cols_cap=1 << 20) == RC_EINVAL   # the u32 column [0, 20) reaches into it
    # with records: a NULL wire, msgs, status or xstat
    for k in ("wire", "msgs", "status", "xstat"):
        assert call(**{k: None}) == RC_EINVAL
        call(**{k: None}, n=0, **trip)
    # the pointer checks come before the alignment checks
    assert call(msgs=C.c_void_p(8), result=None) == RC_EINVAL
    assert call(cols=C.c_void_p(4), xstat=None) == RC_EINVAL
    assert call(present=C.c_void_p(4), rest_pos=p) == RC_EINVAL
    assert call(replies=C.c_void_p(8), flags=2) == RC_EINVAL
    assert call(result=C.c_void_p(4), cols=None) == RC_EINVAL


def _schema_cases():
    F = M.Field
    ok = [F(M.OPAQUE_VAR, 64, 0), F(M.BOOL | M.SELECT, 0, 80), F(M.U64 | M.IF, 0, 120, 1), F(M.U32 | M.NO_COLUMN),
          F(M.OPAQUE_FIXED, 5, 200), F(M.ARRAY32, T, 240), F(M.ARRAY64 | M.IF, 0, 320, T), F(M.U32 | M.SELECT | M.IF, 0, 400, 2)]
    cases = [(ok, 10, 440), (ok, 10, 439), (ok, 0, 400), (ok, 0, 399), ([], 0, 0), ([], 5, 0)]
    bad = [F(7), F(0xFF), F(M.U32 | 0x800), F(M.U32 | 0x80000000), F(M.U32, 0, 0, 0, 1),
           F(M.U64 | M.SELECT), F(M.OPAQUE_FIXED | M.SELECT, 4), F(M.OPAQUE_VAR | M.SELECT, 4), F(M.ARRAY32 | M.SELECT, 4),
           F(M.ARRAY64 | M.SELECT, 4),
           F(M.U32, 0, 0, 1), F(M.U32, 0, 0, T),                  # cond_val without IF
           F(M.U32, 1), F(M.U64, 1), F(M.BOOL, T),                # arg on a type without one
           F(M.U32 | M.NO_COLUMN, 0, 4), F(M.U32 | M.NO_COLUMN, 0, 1 << 63),
           F(M.U32, 0, 2), F(M.U32, 0, 1), F(M.U64, 0, 4), F(M.U64, 0, 12), F(M.OPAQUE_VAR, 9, 6), F(M.BOOL, 0, 3),
           F(M.U32, 0, 2000), F(M.U32, 0, 1 << 63), F(M.U32, 0, (1 << 64) - 4), F(M.U64, 0, (1 << 64) - 8),
           F(M.U32, 0, 964), F(M.U64, 0, 928), F(M.OPAQUE_VAR, 9, 928)]   # the column's end past cols_cap (1000)
    for b in bad:
        for at in (0, 1, 2):
            rows = [F(M.U32, 0, 0), F(M.BOOL | M.SELECT, 0, 40), F(M.U32 | M.IF, 0, 80, 1)]
            rows.insert(at, b._replace(col_off=b.col_off if b.col_off or b.type_flags & M.NO_COLUMN else 120))
            cases.append((rows, 10, 1000))
    good_edges = [F(M.U32, 0, 960), F(M.U64, 0, 920), F(M.OPAQUE_VAR, 0, 920), F(M.U32 | M.NO_COLUMN),
                  F(M.OPAQUE_FIXED, T, 960), F(M.ARRAY64, T, 920)]
    cases += [([g], 10, 1000) for g in good_edges]
    # IF needs an earlier SELECT: not its own, not a later one
    cases.append(([F(M.U32 | M.IF, 0, 0, 1)], 1, 64))
    cases.append(([F(M.U32 | M.IF | M.SELECT, 0, 0, 1)], 1, 64))
    cases.append(([F(M.U32, 0, 0), F(M.U32 | M.IF, 0, 8, 1), F(M.U32 | M.SELECT, 0, 16)], 1, 64))
    cases.append(([F(M.BOOL | M.SELECT, 0, 0), F(M.U32, 0, 8), F(M.U32 | M.IF, 0, 16, 0)], 1, 64))
    # overlap with an earlier column: by one byte range, from either side, with the second half of a pair column,
    # the earlier one first, in the middle and last; touching ranges and empty ones (n == 0) do not overlap
    cases.append(([F(M.U32, 0, 0), F(M.U32, 0, 36)], 10, 1000))
    cases.append(([F(M.U32, 0, 40), F(M.U32, 0, 4)], 10, 1000))
    cases.append(([F(M.U32, 0, 40), F(M.U32, 0, 0)], 10, 1000))
    cases.append(([F(M.OPAQUE_VAR, 9, 0), F(M.U32, 0, 76)], 10, 1000))
    cases.append(([F(M.OPAQUE_VAR, 9, 0), F(M.U32, 0, 80)], 10, 1000))
    cases.append(([F(M.U32, 0, 0), F(M.U32, 0, 40), F(M.U64, 0, 80), F(M.U32, 0, 156)], 10, 1000))
    cases.append(([F(M.U32, 0, 0), F(M.U32, 0, 40), F(M.U64, 0, 80), F(M.U32, 0, 44)], 10, 1000))
    cases.append(([F(M.U32, 0, 0), F(M.U32 | M.NO_COLUMN), F(M.U32, 0, 0)], 10, 1000))
    cases.append(([F(M.U32, 0, 0), F(M.U32, 0, 0), F(M.U64, 0, 0)], 0, 0))
    cases.append(([F(M.U32, 0, 8), F(M.U32, 0, 8)], 1, 1000))
    # two bad fields: the first is reported
    cases.append(([F(M.U32, 0, 0), F(9), F(M.U32, 0, 2)], 1, 64))
    return cases


def test_schema_check_first_bad_field():
    import onc_rpc_amd.runtime as R
    cases = _schema_cases()
    want = [M.schema_check(rows, n, cap) for rows, n, cap in cases]
    got = [R.xdr_schema_check(_fields([tuple(f) for f in rows]), n, cap) for rows, n, cap in cases]
    assert got == want
    assert want[:6] == [0, 8, 0, 8, 0, 0] and want[-1] == 2
    assert {0, 1, 2, 3, 4} <= set(want)
    lib = R.load_library()
    assert lib.onc_xdr_schema_check(None, 1, 0, 0) == RC_EINVAL
    assert lib.onc_xdr_schema_check(None, 0, 0, 0) == 0
    f65 = _fields([(M.U32 | M.NO_COLUMN,)] * 65)
    assert lib.onc_xdr_schema_check(C.c_void_p(f65.ctypes.data), 65, 0, 0) == RC_EINVAL
    assert lib.onc_xdr_schema_check(C.c_void_p(f65.ctypes.data), 64, 0, 0) == 0


def _build_probe(d):
    src = os.path.join(ROOT, "tests", "cpp_xdr", "plan_probe.cpp")
    inc = os.path.join(ROOT, "onc-rpc_amd", "csrc")
    exe = os.path.join(d, "plan_probe_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", inc, src, "-o", exe], check=True,
                   capture_output=True, text=True)
    return exe


@pytest.fixture(scope="module")
def probe():
    with tempfile.TemporaryDirectory() as d:
        exe = _build_probe(d)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

        def run(script):
            r = subprocess.run([exe], input=script, capture_output=True, text=True, timeout=120, env=env)
            assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
            assert "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-3000:]
            return r.stdout.split("\n")[:-1]
        yield run


def _schema_cmd(fields):
    return "S %d\n" % len(fields) + "".join("%d %d %d %d %d\n" % tuple(f) for f in fields)


def _parse_cmd(flags, heads, o, hi, base, L, data):
    return "P %d %d %d %d %d %d %d %s\n" % (flags, int(heads), o, hi, base, L, len(data), data.hex() or "-")


def _parse_want(fields, flags, heads, o, hi, base, L, data):
    def read(p):
        assert p + 4 <= len(data), "the model reads only what it checked"
        return int.from_bytes(data[p:p + 4], "big")
    code, fail, present, p, values = M.parse(read, fields, flags, L, base, o, hi, heads)
    vs = " ".join("%d:%d" % v if isinstance(v, tuple) else "%d" % v for v in values)
    return ("P %d %d %d %d %s" % (code, fail, present, p, vs)).rstrip()


def _check_parses(probe, fields, recs):
    """recs: (flags, heads, o, hi, base, L, data)."""
    out = probe(_schema_cmd(fields) + "".join(_parse_cmd(*r) for r in recs))
    want = [_parse_want(fields, *r) for r in recs]
    assert out == want
    return want


def _codes(want):
    return {int(w.split()[1]) for w in want}


def test_probe_schema_rules(probe):
    cases = _schema_cases()
    script = "".join(_schema_cmd(rows) + "V %d %d\n" % (n, cap) for rows, n, cap in cases if len(rows) <= 64)
    want = ["V %d" % M.schema_check(rows, n, cap) for rows, n, cap in cases if len(rows) <= 64]
    assert probe(script) == want
    # how far the word reads can reach: every field present, every length and count at its maximum
    F = M.Field
    pre = [([], 0), ([F(M.U32), F(M.U64), F(M.BOOL)], 16), ([F(M.U64), F(M.OPAQUE_VAR, 9), F(M.U32)], 28),
           ([F(M.U32), F(M.U32 | M.SELECT), F(M.U32 | M.IF, 0, 0, 1)], 12),
           ([F(M.U32), F(M.OPAQUE_FIXED, 8), F(M.U32)], 16), ([F(M.U32), F(M.OPAQUE_FIXED, 8)], 4),
           ([F(M.ARRAY64, 9)], 4), ([F(M.ARRAY64, T), F(M.U32)], 1000), ([F(M.OPAQUE_VAR, T), F(M.U32)], 1000),
           ([F(M.OPAQUE_VAR, 64), F(M.U64), F(M.U32), F(M.U32), F(M.OPAQUE_VAR, T)], 88), ([F(M.U64)] * 64, 512)]
    assert probe("".join(_schema_cmd(f) + "F 1000\n" for f, _ in pre)) == ["F %d" % b for _, b in pre]
    assert probe("".join(_schema_cmd(f) + "F 65\n" for f, _ in pre)) == ["F %d" % min(b, 65) for _, b in pre]


def test_probe_every_type_with_0_to_12_bytes_left(probe):
    blob = struct.pack(">IIII", 1, 0, 2, 7)
    for t, arg in ((M.U32, 0), (M.U64, 0), (M.BOOL, 0), (M.OPAQUE_FIXED, 0), (M.OPAQUE_FIXED, 1), (M.OPAQUE_FIXED, 4),
                   (M.OPAQUE_FIXED, 5), (M.OPAQUE_FIXED, 8), (M.OPAQUE_FIXED, 9), (M.OPAQUE_VAR, 8), (M.ARRAY32, 2),
                   (M.ARRAY64, 1)):
        # a word in front, so that p > 0, then the field under test, once more behind a taken IF
        for tail in ([M.Field(t, arg)], [M.Field(M.U32 | M.SELECT), M.Field(t | M.IF, arg, 0, 1)]):
            fields = [M.Field(M.U32)] + tail
            recs = []
            for left in range(0, 13):
                for first in (0, 1, 2, 3, 8, 9):                  # the field's first word: a value, a bool, a length
                    data = struct.pack(">I", 5) + (struct.pack(">I", 1) if len(tail) == 2 else b"") + \
                        (struct.pack(">I", first) + blob)[:left]
                    for flags in (0, M.EXACT):
                        recs.append((flags, False, 0, 1 << 40, 7, len(data), data))
            want = _check_parses(probe, fields, recs)
            assert M.OK in _codes(want)
            assert M.SHORT in _codes(want) or (t, arg) == (M.OPAQUE_FIXED, 0)   # (needs no byte)


def test_probe_hostile_lengths_and_counts(probe):
    recs_for = {}
    for t, arg in ((M.OPAQUE_VAR, 16), (M.OPAQUE_VAR, T), (M.OPAQUE_VAR, T - 2), (M.ARRAY32, 3), (M.ARRAY32, T),
                   (M.ARRAY64, 3), (M.ARRAY64, T), (M.ARRAY32, 0x40000000), (M.ARRAY64, 0x20000000)):
        fields = [M.Field(t, arg), M.Field(M.U32)]
        recs = []
        vals = {arg, (arg + 1) & T, arg - 1 if arg else 0, T - 2, T - 1, T, 0x40000000, 0x20000000, 0x80000000, 0, 1}
        for v in sorted(vals):
            for room in (0, 4, 8, 12, 16, 20, 36):
                data = struct.pack(">I", v) + b"\x07" * room
                recs.append((0, False, 0, 1 << 40, 0, len(data), data))
                recs.append((M.EXACT, False, 3, 1 << 40, T - len(data), len(data), data))   # base + L = 0xFFFFFFFF
        want = _check_parses(probe, fields, recs)
        recs_for[(t, arg)] = _codes(want)
        assert {M.SHORT, M.OK} <= _codes(want)
    assert M.TOO_LONG in recs_for[(M.OPAQUE_VAR, 16)] and M.TOO_LONG not in recs_for[(M.OPAQUE_VAR, T)]
    # a count whose byte product is 0 in 32 bits is SHORT, never a zero-byte array
    f32, f64 = [M.Field(M.ARRAY32, T)], [M.Field(M.ARRAY64, T)]
    d32, d64 = struct.pack(">I", 0x40000000) + b"\0" * 8, struct.pack(">I", 0x20000000) + b"\0" * 8
    assert _check_parses(probe, f32, [(0, False, 0, 1 << 40, 0, 12, d32)]) == ["P 3 0 0 0 0:0"]
    assert _check_parses(probe, f64, [(0, False, 0, 1 << 40, 0, 12, d64)]) == ["P 3 0 0 0 0:0"]
    # pad4(0xFFFFFFFD .. 0xFFFFFFFF) is 2^32, not 0
    fv = [M.Field(M.OPAQUE_VAR, T)]
    for v in (T - 2, T - 1, T):
        d = struct.pack(">I", v) + b"\0" * 4
        assert _check_parses(probe, fv, [(0, False, 0, 1 << 40, 0, 8, d)]) == ["P 3 0 0 0 0:0"]
    assert _check_parses(probe, [M.Field(M.OPAQUE_FIXED, T)], [(0, False, 0, 1 << 40, 0, 8, b"\0" * 8)]) == \
        ["P 3 0 0 0 0"]


def test_probe_bool_select_and_heads(probe):
    F = M.Field
    fields = [F(M.BOOL | M.SELECT), F(M.U32 | M.IF, 0, 0, 1), F(M.U32 | M.SELECT), F(M.U64 | M.IF, 0, 0, 2),
              F(M.U32 | M.IF, 0, 0, T), F(M.BOOL | M.SELECT | M.IF, 0, 0, 7), F(M.U32 | M.IF, 0, 0, 1), F(M.U32)]
    recs = []
    for b in (0, 1, 2, T):
        for s in (0, 1, 2, 7, T):
            for inner in (0, 1, 2):
                data = struct.pack(">I", b) + (struct.pack(">I", 11) if b == 1 else b"") + struct.pack(">I", s)
                data += {2: struct.pack(">Q", (1 << 63) + 9), T: struct.pack(">I", 12)}.get(s, b"")
                data += struct.pack(">I", inner) if s == 7 else b""
                data += struct.pack(">I", 13) if (s == 7 and inner == 1) else b""
                data += struct.pack(">I", 14)
                for cut in (len(data), len(data) - 1, len(data) + 4):
                    d = (data + b"\x55" * 4)[:cut]
                    recs.append((M.EXACT, False, 0, 1 << 40, 0, len(d), d))
    want = _check_parses(probe, fields, recs)
    assert {M.OK, M.BAD_BOOL, M.SHORT, M.TRAILING} <= _codes(want)
    # the heads form: a word that ends past the head is HEAD_SHORT, a body that does is not looked at
    fields = [F(M.OPAQUE_VAR, 64), F(M.U64), F(M.U32)]
    data = struct.pack(">I", 9) + b"\x01" * 12 + struct.pack(">QI", 77, 5)
    recs = []
    for room in range(0, len(data) + 2):                       # bytes of the payload inside the head
        recs.append((0, True, 100, 100 + room, 36, len(data), data[:room]))
    want = _check_parses(probe, fields, recs)
    assert _codes(want) == {M.OK, M.HEAD_SHORT}


def test_probe_extents(probe):
    H = 1 << 32
    cases = []
    for L in (0, 1, 100, T):
        for base in (0, 1, T - L - 1, T - L, T - L + 1, H - L, H, H + 5):
            if base < 0:
                continue
            # rec_start form: o - start = base, inside a huge wire
            cases.append((1000 + base, L, 0, 0, 0, 1, 1000, 1 << 62))
            # heads form: base is at most head_len
            cases.append((5 * 4096 + min(base, 4097), L, 5, 1, 4096, 0, 0, 1 << 62))
    for o, L, wl in ((10, 0, 10), (11, 0, 10), (0, 11, 10), (5, 6, 10), (5, 5, 10), ((1 << 64) - 1, 1, 10),
                     ((1 << 64) - 1, 0, (1 << 64) - 1), ((1 << 64) - 1, 1, (1 << 64) - 1), (7, T, (1 << 64) - 1)):
        for has_start, start in ((0, 0), (1, 0), (1, o), (1, o + 1 if o + 1 < 1 << 64 else o), (1, 3)):
            cases.append((o, L, 0, 0, 0, has_start, start, wl))
    script, want = "", []
    for o, L, r, heads, head_len, has_start, start, wl in cases:
        script += "X %d %d %d %d %d %d %d %d\n" % (o, L, r, heads, head_len, has_start, start, wl)
        if heads:
            lo = r * head_len
            hi = lo + head_len
            bad, base = o < lo or o > hi, o - lo
        else:
            hi = wl
            bad = o > wl or L > wl - o
            base = o - start if has_start else 0
            bad = bad or (has_start and o < start)
        bad = bad or base + L > T
        want.append("X %d %d %d" % (int(bad), 0 if bad else base, hi))
    out = probe(script)
    assert out == want
    assert any(w.startswith("X 0") for w in want) and any(w.startswith("X 1") for w in want)


def test_cpp_mirror_program_compiles():
    """XdrSchema, unpack_args and UnpackedArgs (include/onc_rpc.hpp) build
    against the C ABI (build() compiles tests/cpp_xdr)."""
    exe = os.path.join(ROOT, "tests", "cpp_xdr", "test_xdr")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "include", "onc_rpc.hpp")).read()
    assert "onc_xdr_unpack" in hpp and "XdrSchema" in hpp and "unpack_args" in hpp and "UnpackedArgs" in hpp
