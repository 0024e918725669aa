"""CPU tests of onc_fragment (records cut into fragments on the send side):
the symbol and its argument checks, and the record arithmetic the kernels
call (onc-rpc_amd/csrc/fragment_plan.h) at the extremes of its 64-bit
arguments — a body of 2^31 or 2^40 bytes cannot be given to a GPU test, so
its fragment count, length, marks and position map are checked here, in a
stand-alone host program."""
import ctypes as C
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL = -1


def test_fragment_symbol_and_argument_checks():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    assert lib.onc_abi_version() == 8 == R.ABI_VERSION      # additive: callers find the symbol by linking
    assert R.K_COUNT == 16
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and "#define ONC_K_COUNT        16" in hdr
    assert hasattr(C.CDLL(LIB), "onc_fragment") and "onc_fragment" in R.EXPORTED
    fake = C.c_void_p(8)                             # never dereferenced: the checks come first
    p = C.c_void_p(16)
    f = lib.onc_fragment
    # NULL codec, out_off or result, whatever n is
    for n in (0, 1):
        assert f(None, p, p, n, 16, p, 64, p, p, p) == RC_EINVAL
        assert f(fake, p, p, n, 16, p, 64, None, p, p) == RC_EINVAL
        assert f(fake, p, p, n, 16, p, 64, p, p, None) == RC_EINVAL
        # max_frag outside 1 .. 0x7FFFFFFF
        assert f(fake, p, p, n, 0, p, 64, p, p, p) == RC_EINVAL
        assert f(fake, p, p, n, 0x80000000, p, 64, p, p, p) == RC_EINVAL
        assert f(fake, p, p, n, 0xFFFFFFFF, p, 64, p, p, p) == RC_EINVAL
    # with records: NULL wire, offsets, status, or out with a capacity
    assert f(fake, None, p, 1, 16, p, 64, p, p, p) == RC_EINVAL
    assert f(fake, p, None, 1, 16, p, 64, p, p, p) == RC_EINVAL
    assert f(fake, p, p, 1, 16, p, 64, p, None, p) == RC_EINVAL
    assert f(fake, p, p, 1, 16, None, 64, p, p, p) == RC_EINVAL


def test_n_zero_is_accepted_by_the_argument_checks():
    """n == 0 needs no wire, offsets, status or out: the call gets past its
    argument checks (on a machine without a GPU a handle cannot be made, and
    a NULL one is refused first)."""
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    h = C.c_void_p()
    if lib.onc_codec_create(C.byref(h), 0, None) == 0:          # a GPU is here: the real thing
        import torch
        out_off = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        res = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        for max_frag in (1, 0x7FFFFFFF):
            assert lib.onc_fragment(h, None, None, 0, max_frag, None, 0, C.c_void_p(out_off.data_ptr()), None,
                                    C.c_void_p(res.data_ptr())) == 0
        lib.onc_codec_sync(h)
        assert out_off.item() == 0 and not res.cpu().numpy().any()
        lib.onc_codec_destroy(h)
    else:
        assert lib.onc_fragment(None, None, None, 0, 16, None, 0, C.c_void_p(16), None, C.c_void_p(16)) == RC_EINVAL


def test_plan_arithmetic_extremes():
    """fragment_plan.h compiled by the host compiler into a stand-alone
    program (tests/cpp_fragment/plan_probe.cpp), with the undefined-behaviour
    sanitizer where the toolchain links it: bodies around max_frag and its
    multiples, of 2^31 - 1, 2^31 and 2^40 bytes at max_frag 1 and 0x7FFFFFFF,
    extents of 0, 1, 3 and 4 bytes, out_cap = 0, positions near 2^64 against
    the capacity (no wrap), the position map against a brute-force walk, and
    the plan's scan at every blocking of a record list."""
    src = os.path.join(ROOT, "tests", "cpp_fragment", "plan_probe.cpp")
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
    assert r.stdout.strip() == "fragment plan ok"


def test_cpp_mirror_program_compiles():
    """fragment_stream (include/onc_rpc.hpp) builds against the C ABI
    (build() compiles tests/cpp_fragment)."""
    exe = os.path.join(ROOT, "tests", "cpp_fragment", "test_fragment")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    assert "onc_fragment" in open(os.path.join(ROOT, "include", "onc_rpc.hpp")).read()
