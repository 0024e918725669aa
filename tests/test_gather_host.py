"""CPU tests of onc_piece_offsets / onc_gather_pieces (a piece list written as
one stream on the device): the symbols and their argument checks, and the
arithmetic the kernels call (onc-rpc_amd/csrc/gather_plan.h) in a stand-alone
host program — which pieces may be read near 2^64 and at a source's end, what
is left of a window whose end wraps, and the offsets' scan at every blocking
of a short list."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL, RC_EALIGN = -1, -4


def _src(R, bases=(64, 64, 64), lens=(8, 8, 8)):
    s = R.OncGatherSrc()
    for k in range(3):
        s.base[k] = bases[k]
        s.len[k] = lens[k]
    return s


def test_gather_symbols_and_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8 == R.ABI_VERSION      # additive: callers find the symbols by linking
    assert R.K_COUNT == 16 and len(R.K_NAMES) == 16
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and "#define ONC_K_COUNT        16" in hdr
    raw = C.CDLL(LIB)
    for name in ("onc_piece_offsets", "onc_gather_pieces"):
        assert hasattr(raw, name) and name in R.EXPORTED and name in hdr
    assert hasattr(R.Codec, "piece_offsets") and hasattr(R.Codec, "gather_pieces")
    assert C.sizeof(R.OncGatherSrc) == 48
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p = C.c_void_p(16)
    src = C.byref(_src(R))
    po, ga = lib.onc_piece_offsets, lib.onc_gather_pieces
    # NULL codec, src, piece_pos or result, whatever npieces is
    for n in (0, 1):
        assert po(None, p, n, src, p, p) == RC_EINVAL
        assert po(fake, p, n, None, p, p) == RC_EINVAL
        assert po(fake, p, n, src, None, p) == RC_EINVAL
        assert po(fake, p, n, src, p, None) == RC_EINVAL
        for count in (0, 5):
            assert ga(None, p, p, n, src, 0, count, p) == RC_EINVAL
            assert ga(fake, p, p, n, None, 0, count, p) == RC_EINVAL
            assert ga(fake, p, None, n, src, 0, count, p) == RC_EINVAL
        # NULL out with bytes asked for
        assert ga(fake, p, p, n, src, 0, 1, None) == RC_EINVAL
        assert ga(fake, p, p, n, src, 1 << 63, (1 << 64) - 1, None) == RC_EINVAL
    # NULL pieces with pieces to read
    assert po(fake, None, 1, src, p, p) == RC_EINVAL
    assert ga(fake, None, p, 1, src, 0, 4, p) == RC_EINVAL
    # a source with bytes and no base, each of the three; NULL with len 0 is fine (checked below)
    for k in range(3):
        bases = [64, 64, 64]
        bases[k] = None
        bad = C.byref(_src(R, bases))
        for n in (0, 1):
            assert po(fake, p, n, bad, p, p) == RC_EINVAL
            assert ga(fake, p, p, n, bad, 0, 4, p) == RC_EINVAL
    # pieces not 16-byte aligned, piece_pos not 8-byte aligned (the source check passes: len 0 with NULL)
    empty = C.byref(_src(R, (None, 64, None), (0, 8, 0)))
    for s in (src, empty):
        for a in (8, 24, 36, 17):
            assert po(fake, C.c_void_p(a), 1, s, p, p) == RC_EALIGN
            assert ga(fake, C.c_void_p(a), p, 1, s, 0, 4, p) == RC_EALIGN
        for a in (4, 12, 17, 20):
            assert po(fake, p, 1, s, C.c_void_p(a), p) == RC_EALIGN
            assert ga(fake, p, C.c_void_p(a), 1, s, 0, 4, p) == RC_EALIGN
    # the pointer checks come before the alignment checks
    assert po(fake, C.c_void_p(8), 1, src, p, None) == RC_EINVAL
    assert ga(fake, C.c_void_p(8), p, 1, src, 0, 4, None) == RC_EINVAL


def test_no_pieces_and_no_bytes():
    """npieces == 0 needs no pieces and count == 0 no out. With a GPU:
    piece_pos[0] = 0, the result {0, 0, 0}, and gathers that write nothing.
    Without one no handle can be made, and a NULL one is refused first: the
    calls get past every other argument check."""
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    h = C.c_void_p()
    src = _src(R, (None, None, None), (0, 0, 0))
    if lib.onc_codec_create(C.byref(h), 0, None) == 0:          # a GPU is here: the real thing
        import torch
        pos = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
        pp, rp, op = (C.c_void_p(t.data_ptr()) for t in (pos, res, out))
        assert lib.onc_piece_offsets(h, None, 0, C.byref(src), pp, rp) == 0
        assert lib.onc_gather_pieces(h, None, pp, 0, C.byref(src), 0, 64, op) == 0
        assert lib.onc_gather_pieces(h, None, pp, 0, C.byref(src), 0, 0, None) == 0
        # one piece, no bytes asked for
        piece = torch.zeros(16, dtype=torch.uint8, device="cuda")
        assert lib.onc_gather_pieces(h, C.c_void_p(piece.data_ptr()), pp, 1, C.byref(src), 0, 0, None) == 0
        lib.onc_codec_sync(h)
        assert pos.tolist() == [0, -1] and res.tolist() == [0, 0, 0, -1]
        assert (out == 0xA5).all().item()
        lib.onc_codec_destroy(h)
    else:
        p = C.c_void_p(16)
        assert lib.onc_piece_offsets(None, None, 0, C.byref(src), p, p) == RC_EINVAL
        assert lib.onc_gather_pieces(None, None, p, 0, C.byref(src), 0, 0, None) == RC_EINVAL


def test_plan_arithmetic_extremes():
    """gather_plan.h compiled by the host compiler into a stand-alone program
    (tests/cpp_gather/plan_probe.cpp), with the undefined-behaviour sanitizer
    where the toolchain links it: ok() at off = 2^64 - 1 with len = 2, at
    off = len[src] with len 0 and 1, at src = 3; the window at from + count
    wrapping past 2^64 and at from = the stream's end; the scan at every
    blocking of a short list."""
    src = os.path.join(ROOT, "tests", "cpp_gather", "plan_probe.cpp")
    inc = os.path.join(ROOT, "onc-rpc_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plan_probe")
        base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, src, "-o", exe]
        san = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"],
                             capture_output=True, text=True)
        if san.returncode != 0:                      # no sanitizer runtime here: the plain build
            subprocess.run(base, check=True, capture_output=True, text=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "gather plan ok"


def test_cpp_mirror_program_compiles():
    """BatchEncoder::serialise_fragmented and VectoredStream::gather_window
    (include/onc_rpc.hpp) build against the C ABI (build() compiles
    tests/cpp_gather)."""
    exe = os.path.join(ROOT, "tests", "cpp_gather", "test_gather")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    hpp = open(os.path.join(ROOT, "include", "onc_rpc.hpp")).read()
    assert "onc_gather_pieces" in hpp and "serialise_fragmented" in hpp and "gather_window" in hpp
