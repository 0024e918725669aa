"""CPU tests of onc_fragment_iov (the vectored encode's records cut into
fragments without a copy): the symbol and its argument checks, and the record
arithmetic the kernels call (onc-rpc_amd/csrc/fragment_iov_plan.h) in a
stand-alone host program — the piece map against a brute-force walk, entries
of 2^32 - 1 header and payload bytes, both capacities near 2^64. (On the GPU
tests/test_gpu_far_offsets.py gives the kernels entries of 4 GiB payloads;
the capacities near 2^64 stay here.)"""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL, RC_EALIGN = -1, -4


def test_fragment_iov_symbol_and_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8 == R.ABI_VERSION      # additive: callers find the symbol by linking
    assert R.K_COUNT == 16
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and "#define ONC_K_COUNT        16" in hdr
    assert hasattr(C.CDLL(LIB), "onc_fragment_iov") and "onc_fragment_iov" in R.EXPORTED
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p = C.c_void_p(16)
    f = lib.onc_fragment_iov
    # NULL codec, out_off, piece_off or result, and an invalid max_frag, whatever n is
    for n in (0, 1):
        assert f(None, p, n, 16, None, p, 64, p, 4, p, p, p, p) == RC_EINVAL
        assert f(fake, p, n, 16, None, p, 64, p, 4, None, p, p, p) == RC_EINVAL
        assert f(fake, p, n, 16, None, p, 64, p, 4, p, None, p, p) == RC_EINVAL
        assert f(fake, p, n, 16, None, p, 64, p, 4, p, p, p, None) == RC_EINVAL
        for bad in (0, 0x80000000, 0xFFFFFFFF):
            assert f(fake, p, n, bad, None, p, 64, p, 4, p, p, p, p) == RC_EINVAL
            assert f(fake, p, n, bad, p, p, 64, p, 4, p, p, p, p) == RC_EINVAL    # ignored, but must be valid
    # with records: NULL iov or status, NULL marks or pieces with a capacity
    assert f(fake, None, 1, 16, None, p, 64, p, 4, p, p, p, p) == RC_EINVAL
    assert f(fake, p, 1, 16, None, p, 64, p, 4, p, p, None, p) == RC_EINVAL
    assert f(fake, p, 1, 16, None, None, 64, p, 4, p, p, p, p) == RC_EINVAL
    assert f(fake, p, 1, 16, None, p, 64, None, 4, p, p, p, p) == RC_EINVAL
    # marks not 4-byte aligned, pieces not 16-byte aligned
    for a in (17, 18, 19):
        assert f(fake, p, 1, 16, None, C.c_void_p(a), 64, p, 4, p, p, p, p) == RC_EALIGN
    for a in (8, 24, 36, 17):
        assert f(fake, p, 1, 16, None, p, 64, C.c_void_p(a), 4, p, p, p, p) == RC_EALIGN
    assert f(fake, p, 1, 16, None, C.c_void_p(20), 64, C.c_void_p(8), 4, p, p, p, p) == RC_EALIGN


def test_n_zero_is_accepted_by_the_argument_checks():
    """n == 0 needs no iov, status, marks or pieces: the call gets past its
    argument checks (on a machine without a GPU a handle cannot be made, and
    a NULL one is refused first)."""
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    h = C.c_void_p()
    if lib.onc_codec_create(C.byref(h), 0, None) == 0:          # a GPU is here: the real thing
        import torch
        out_off = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        piece_off = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        res = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        for max_frag in (1, 0x7FFFFFFF):
            assert lib.onc_fragment_iov(h, None, 0, max_frag, None, None, 0, None, 0, C.c_void_p(out_off.data_ptr()),
                                        C.c_void_p(piece_off.data_ptr()), None, C.c_void_p(res.data_ptr())) == 0
        lib.onc_codec_sync(h)
        assert out_off.item() == 0 and piece_off.item() == 0 and not res.cpu().numpy().any()
        lib.onc_codec_destroy(h)
    else:
        p = C.c_void_p(16)
        assert lib.onc_fragment_iov(None, None, 0, 16, None, None, 0, None, 0, p, p, None, p) == RC_EINVAL


def test_plan_arithmetic_extremes():
    """fragment_iov_plan.h compiled by the host compiler into a stand-alone
    program (tests/cpp_fragment_iov/plan_probe.cpp), with the
    undefined-behaviour sanitizer where the toolchain links it: the piece map
    against a brute-force walk for every header and payload below 40 bytes at
    every limit below 45, hdr_len = payload_len = 0xFFFFFFFF at limits 1 and
    0x7FFFFFFF, positions near 2^64 against both capacities (no wrap),
    capacities 0, and the plan's scan at every blocking of a record list."""
    src = os.path.join(ROOT, "tests", "cpp_fragment_iov", "plan_probe.cpp")
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
    assert r.stdout.strip() == "fragment iov plan ok"


def test_cpp_mirror_program_compiles():
    """BatchEncoder::serialise_vectored (include/onc_rpc.hpp) builds against
    the C ABI (build() compiles tests/cpp_fragment_iov)."""
    exe = os.path.join(ROOT, "tests", "cpp_fragment_iov", "test_fragment_iov")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    assert "onc_fragment_iov" in open(os.path.join(ROOT, "include", "onc_rpc.hpp")).read()
