"""CPU tests of onc_defragment_heads and onc_decode_heads: the symbols, the
header's promises (ABI 8, sixteen timing ids, the new reason and span, both
functions declared and documented, the serial loop written down), the argument
checks that are made before any GPU call, and the plan arithmetic driven by a
stand-alone host program."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "onc-rpc_amd", "libonc_rpc_amd.so")
RC_EINVAL, RC_EALIGN = -1, -4
NAMES = ("onc_defragment_heads", "onc_decode_heads")


def test_symbols_exported_and_bound():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    raw = C.CDLL(LIB)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in R.EXPORTED
        assert getattr(lib, name).argtypes is not None, name
    assert len(lib.onc_defragment_heads.argtypes) == 13 and len(lib.onc_decode_heads.argtypes) == 7
    for meth in ("defragment_heads", "decode_heads"):
        assert callable(getattr(R.Codec, meth))
    for fn in ("defragment_host_heads", "decode_host_heads"):
        assert callable(getattr(R, fn))


def test_header_keeps_abi_and_documents_the_calls():
    import onc_rpc_amd.layout as L
    import onc_rpc_amd.runtime as R
    hdr = open(os.path.join(ROOT, "include", "onc_rpc.h")).read()
    lib = R.load_library()
    assert "#define ONC_RPC_ABI_VERSION 8" in hdr and lib.onc_abi_version() == 8
    assert re.search(r"#define ONC_K_COUNT\s+16\b", hdr) and R.K_COUNT == 16 == len(R.K_NAMES)
    assert lib.onc_status_str(107) == b"unknown status"            # no new status code
    assert re.search(r"#define ONC_EXTENT_HEAD_SHORT\s+4\b", hdr) and L.EXTENT_HEAD_SHORT == 4
    assert re.search(r"#define ONC_HEAD_SPAN_MAX\s+724\b", hdr) and L.HEAD_SPAN_MAX == 724
    assert 4 + 24 + 2 * (8 + 4 + 4 + 256 + 12 + 64) == 724
    ext = open(os.path.join(ROOT, "onc-rpc_amd", "csrc", "extent.h")).read()
    assert re.search(r"kExtentHeadShort\s*=\s*4;", ext)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int %s\(onc_codec\* codec," % name, code, flags=re.M), name
    # both are on the list of what was added without a version change
    added = hdr[hdr.index("Added without a version change"):hdr.index("#define ONC_RPC_ABI_VERSION")]
    for name in NAMES:
        assert name in added, name
    # the ids the new launches report under are written down next to the id list
    ids = hdr[hdr.index("Per-kernel event timing"):hdr.index("#define ONC_K_ENC_LEN")]
    for word in NAMES + ("heads_place", "heads_gather", "ONC_K_DEFRAG_PLAN", "ONC_K_DEFRAG_COPY", "ONC_K_DEC_PARSE"):
        assert word in ids, word
    # the serial loop is in the header
    for line in ("frag_pre[j] = B",
                 "B += frag_len[j] - 4",
                 "if wire[frag_start[j]] & 0x80:",
                 "if B >= 2^31: rec_len[r] = 0; status[r] = ONC_ENC_TOO_LONG",
                 "status[r] = r < max_records ? ONC_OK : ONC_ENC_WRITE_ZERO",
                 "slot[0, 4) = BE32(0x80000000 | B)",
                 "multi += (j > first); r++; first = j + 1; B = 0",
                 "result = {r, first, r * head_len, nfrag - first, B, multi}"):
        assert line in hdr, line


def test_argument_checks_before_any_gpu_call():
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    fake = C.c_void_p(8)                             # never dereferenced: the checks below come first
    p = C.c_void_p(16)                               # a non-NULL 16-byte aligned array, never dereferenced either
    odd = C.c_void_p(24)
    dh, de = lib.onc_defragment_heads, lib.onc_decode_heads
    # onc_defragment_heads: NULL codec, rec_frag or result whatever nfrag is
    assert dh(None, p, p, p, 1, 160, p, 1, p, p, p, p, p) == RC_EINVAL
    assert dh(fake, p, p, p, 1, 160, p, 1, p, None, p, p, p) == RC_EINVAL
    assert dh(fake, p, p, p, 1, 160, p, 1, p, p, p, p, None) == RC_EINVAL
    assert dh(fake, p, p, p, 0, 160, p, 1, p, None, p, p, p) == RC_EINVAL
    assert dh(fake, p, p, p, 0, 160, p, 1, p, p, p, p, None) == RC_EINVAL
    # with fragments: NULL wire, frag_start, frag_len, rec_len, frag_pre, status
    assert dh(fake, None, p, p, 1, 160, p, 1, p, p, p, p, p) == RC_EINVAL
    assert dh(fake, p, None, p, 1, 160, p, 1, p, p, p, p, p) == RC_EINVAL
    assert dh(fake, p, p, None, 1, 160, p, 1, p, p, p, p, p) == RC_EINVAL
    assert dh(fake, p, p, p, 1, 160, p, 1, None, p, p, p, p) == RC_EINVAL
    assert dh(fake, p, p, p, 1, 160, p, 1, p, p, None, p, p) == RC_EINVAL
    assert dh(fake, p, p, p, 1, 160, p, 1, p, p, p, None, p) == RC_EINVAL
    # NULL heads with slots to fill; head_len; alignment
    assert dh(fake, p, p, p, 1, 160, None, 1, p, p, p, p, p) == RC_EINVAL
    for bad in (0, 16, 48, 63, 65, 72, 168, 4095, 4112, 8192, 0xFFFFFFF0):
        assert dh(fake, p, p, p, 1, bad, p, 1, p, p, p, p, p) == RC_EINVAL, bad
        assert de(fake, p, bad, p, 1, 0, C.byref(R.OncDecoded(16, 16, 16, 16, 16))) == RC_EINVAL, bad
    assert dh(fake, p, p, p, 1, 160, odd, 1, p, p, p, p, p) == RC_EALIGN
    assert dh(fake, p, p, p, 1, 64, C.c_void_p(17), 1, p, p, p, p, p) == RC_EALIGN
    # onc_decode_heads: NULL codec / out, a bad mode, alignment, NULL arrays with records
    d = R.OncDecoded(16, 16, 16, 16, 16)
    assert de(None, p, 160, p, 1, 0, C.byref(d)) == RC_EINVAL
    assert de(fake, p, 160, p, 1, 0, None) == RC_EINVAL
    assert de(fake, p, 160, p, 1, 2, C.byref(d)) == RC_EINVAL
    assert de(fake, odd, 160, p, 1, 0, C.byref(d)) == RC_EALIGN
    assert de(fake, None, 160, p, 1, 0, C.byref(d)) == RC_EINVAL
    assert de(fake, p, 160, None, 1, 0, C.byref(d)) == RC_EINVAL
    assert de(fake, p, 160, p, 1, 0, C.byref(R.OncDecoded(16, 16, None, 16, 16))) == RC_EINVAL
    assert de(fake, p, 160, p, 0, 0, C.byref(d)) == 0                 # no records: nothing to do


def test_nfrag_zero_is_accepted_by_the_argument_checks():
    """nfrag == 0 needs no wire, extents, lengths, status or heads: the call
    gets past its argument checks (on a machine without a GPU no handle can be
    made, and a NULL one is refused first)."""
    import onc_rpc_amd.runtime as R
    lib = R.load_library()
    h = C.c_void_p()
    if lib.onc_codec_create(C.byref(h), 0, None) == 0:
        import torch
        rec_frag = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        res = torch.full((7,), -1, dtype=torch.int64, device="cuda")
        assert lib.onc_defragment_heads(h, None, None, None, 0, 160, None, 0, None, C.c_void_p(rec_frag.data_ptr()),
                                        None, None, C.c_void_p(res.data_ptr())) == 0
        lib.onc_codec_sync(h)
        assert rec_frag.tolist() == [0, -1] and res.tolist() == [0] * 6 + [-1]
        lib.onc_codec_destroy(h)
    else:
        assert lib.onc_defragment_heads(None, None, None, None, 0, 160, None, 0, None, C.c_void_p(16), None, None,
                                        C.c_void_p(16)) == RC_EINVAL


def test_plan_arithmetic_extremes():
    """defrag_heads_plan.h compiled by the host compiler into a stand-alone
    program (tests/cpp_heads/plan_probe.cpp), with the address and
    undefined-behaviour sanitizers where the toolchain links them: B_r =
    2^31 - 1 (OK) and 2^31 (TOO_LONG), the capacity cut by record index, the
    result words, pending fragments, the scan at every blocking, and the
    fragment search against a walk with runs of empty fragments."""
    src = os.path.join(ROOT, "tests", "cpp_heads", "plan_probe.cpp")
    inc = os.path.join(ROOT, "onc-rpc_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "plan_probe")
        base = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", inc, src, "-o", exe]
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                             capture_output=True, text=True)
        if san.returncode != 0:                      # no sanitizer runtime here: the plain build
            subprocess.run(base, check=True, capture_output=True, text=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "defrag heads plan ok"


def test_cpp_mirror_program_compiles():
    """reassemble_heads and BatchDecoder::try_from_fragmented_heads
    (include/onc_rpc.hpp) build against the C ABI (build() compiles
    tests/cpp_heads)."""
    exe = os.path.join(ROOT, "tests", "cpp_heads", "test_heads")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.dirname(exe)], check=True, capture_output=True, timeout=600)
    assert os.path.exists(exe)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '"tests/cpp_heads"' in entry
