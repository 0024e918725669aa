"""CPU tests of the bounded decode (onc_decode_bounded,
onc_decode_lengths_bounded, onc_decode_body_bounded): the symbols and their
argument checks, the new status' text, and the extent predicate the kernels
call (onc-rpc_amd/csrc/extent.h) at the extremes of its 64-bit arguments —
the arithmetic is checked here, in a stand-alone host program, and extreme
offsets are never handed to the GPU."""
import ctypes as C
import os
import subprocess
import tempfile

import onc_rpc_amd.layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL = -1


def test_bounded_symbols_and_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8               # additive: callers find the symbols by linking
    for name in ("onc_decode_bounded", "onc_decode_lengths_bounded", "onc_decode_body_bounded"):
        assert hasattr(C.CDLL(LIB), name), name
        assert name in R.EXPORTED
    out = R.OncDecoded(0, 0, 0, 0, 0)
    # a NULL codec, a NULL out, a bad mode: refused as by the unbounded
    # calls, before any GPU call (this machine has none)
    assert lib.onc_decode_bounded(None, None, 0, None, 1, L.DECODE_SLICE, C.byref(out)) == RC_EINVAL
    assert lib.onc_decode_lengths_bounded(None, None, 0, None, 1, 0, L.DECODE_SLICE, None, C.byref(out)) == RC_EINVAL
    assert lib.onc_decode_body_bounded(None, L.ROOT_OPAQUE, None, 0, None, 1, L.DECODE_SLICE, None, C.byref(out),
                                       None) == RC_EINVAL
    fake = C.c_void_p(8)                             # never dereferenced: the checks below come first
    assert lib.onc_decode_bounded(fake, None, 0, None, 1, L.DECODE_SLICE, None) == RC_EINVAL
    assert lib.onc_decode_bounded(fake, None, 0, None, 1, 7, C.byref(out)) == RC_EINVAL
    assert lib.onc_decode_lengths_bounded(fake, None, 0, None, 1, 0, 7, None, C.byref(out)) == RC_EINVAL
    assert lib.onc_decode_body_bounded(fake, 99, None, 0, None, 1, L.DECODE_SLICE, None, C.byref(out),
                                       None) == RC_EINVAL
    assert lib.onc_decode_bounded(fake, None, 0, None, 1, L.DECODE_SLICE, C.byref(out)) == RC_EINVAL  # NULL arrays
    assert lib.onc_decode_lengths_bounded(fake, None, 0, None, 1, 0, L.DECODE_SLICE, None,
                                          C.byref(out)) == RC_EINVAL
    assert lib.onc_decode_bounded(fake, None, 0, None, 0, L.DECODE_SLICE, C.byref(out)) == 0          # n = 0


def test_bad_extent_status():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert L.DEC_BAD_EXTENT == 106
    assert (L.EXTENT_START_PAST_WIRE, L.EXTENT_END_PAST_WIRE, L.EXTENT_NOT_MONOTONIC) == (1, 2, 3)
    assert L.STATUS[106] == "DecBadExtent"
    assert lib.onc_status_str(106) == b"slice index out of range: record extent outside the wire"
    assert lib.onc_status_str(105) == b"failed to write whole buffer"        # neighbours untouched
    assert lib.onc_status_str(107) == b"unknown status"
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_DEC_BAD_EXTENT      106" in hdr


def test_extent_predicate_extremes():
    """extent.h compiled by the host compiler into a stand-alone program
    (tests/cpp_bounded/extent_probe.cpp), with the undefined-behaviour
    sanitizer where the toolchain links it: b = wire_len with L = 0 (ok) and
    L = 1 (end), b = wire_len + 1 (start), b = 2^64 - 8 with L = 16 (start: no
    wrap), the offsets pair (100, 50) (order), wire_len = 0."""
    src = os.path.join(ROOT, "tests", "cpp_bounded", "extent_probe.cpp")
    inc = os.path.join(ROOT, "onc-rpc_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "extent_probe")
        base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, src, "-o", exe]
        san = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"],
                             capture_output=True, text=True)
        if san.returncode != 0:                      # no sanitizer runtime here: the plain build
            subprocess.run(base, check=True, capture_output=True, text=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "extent ok"
